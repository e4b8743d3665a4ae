// jellyfish_amd/csrc/abi_sorted.inl -- C ABI of the look-ups in a binary/sorted body (jfgpu_sorted_*), included by jfgpu.hip.
// Kernels: kernels_sorted.hip.hpp.  The object owns its stream, the body as the file has it, the bucket index over it and the
// matrix's byte tables (hip_own.hpp); SortedView, what the kernels get, points into them (view()).  The body goes up in windows
// through the pinned staging of a WindowPipe, as jfgpu_text_run and jfgpu_merge_run upload theirs, into one device buffer.
struct jfgpu_sorted {
  int device = 0, n_cu = 256;
  Stream stream;                 // (before the buffers used on it: they go first)
  uint32_t k = 0, kb = 0, kw = 0, vb = 0, rb = 0, key_bits = 0, lsize = 0, bucket_bits = 0;
  uint64_t size = 0, n_records = 0, longest = 0, device_bytes = 0, upload_us = 0, index_us = 0;
  TableGeom g{};                 // only k / key_mask / canonical / nbytes are used (the views that roll the k-mers)
  bool wide = false; WideGeom wg{};   // 33 <= k <= 64: two-word keys
  bool nword = false; NGeom ng{};     // 65 <= k <= 128: keys of three and four words
  DevBuf<uint8_t> d_body;
  DevBuf<uint64_t> d_index, d_fwd;
  DevBuf<uint8_t> d_stage;       // jfgpu_sorted_query_ascii: a piece of the caller's bases
  SortedView view() const {
    SortedView v;
    v.body = d_body; v.index = d_index; v.fwd = d_fwd; v.n_records = n_records; v.pos_mask = size - 1;
    v.val_mask = vb >= 8 ? ~0ull : ((1ull << (8 * vb)) - 1);
    v.rb = rb; v.kb = kb; v.key_bits = key_bits; v.bucket_shift = lsize - bucket_bits;
    return v;
  }
};

namespace {

constexpr uint32_t kSortedRecordsPerBucket = 8;
constexpr size_t kSortedUploadWindow = (size_t)16 << 20;   // bytes of the body staged and copied at a time

int use_s(const jfgpu_sorted* s) { return use_dev(s, "null sorted records"); }

// what plan and create refuse alike; *lsize = log2(size)
int sorted_args(uint64_t n_records, uint64_t size, uint32_t k, uint32_t counter_len, uint32_t* lsize) {
  if(k > 128) return fail(JFGPU_E_UNSUPPORTED, "sorted: mer length > 128 (more than four key words) is not built");
  if(counter_len > 8) return fail(JFGPU_E_UNSUPPORTED, "sorted: counter_len > 8 is not built");
  if(k < 1) return fail(JFGPU_E_INVALID, "sorted: mer length must be >= 1");
  if(counter_len < 1) return fail(JFGPU_E_INVALID, "sorted: counter_len must be in [1, 8]");
  if(size == 0 || (size & (size - 1))) return fail(JFGPU_E_INVALID, "sorted: size must be a power of two");
  if(n_records >= ((uint64_t)1 << 39)) return fail(JFGPU_E_UNSUPPORTED, "sorted: 2^39 records or more (the index kernel's tiles are a 32-bit grid)");
  uint32_t l = 0;
  while(((uint64_t)1 << l) != size) ++l;
  *lsize = l;
  return JFGPU_OK;
}

template <int KW>
void sorted_launch_index(jfgpu_sorted* s, const SortedView& V, uint32_t* d_flag) {
  const uint64_t tiles = (s->n_records + kMergeBlock - 1) / kMergeBlock;
  hipLaunchKernelGGL((sorted_index_kernel<KW>), dim3((unsigned)tiles), dim3(kMergeBlock), 0, s->stream, V, (uint64_t)1 << s->bucket_bits, d_flag);
}

template <int KW>
void sorted_launch_lookup(jfgpu_sorted* s, int grid, const uint64_t* d_keys, uint64_t n, uint64_t* d_vals, uint8_t* d_found) {
  hipLaunchKernelGGL((sorted_lookup_kernel<KW>), dim3(grid), dim3(kBlock), 0, s->stream, s->view(), d_keys, n, d_vals, d_found);
}

// The body into d_body, a window at a time: window i is staged in pinned memory (the page-cache reads) while the copy of
// window i - 1 runs.  A slot's staging buffer is refilled only after its last copy has ended.
int sorted_upload(jfgpu_sorted* s, const uint8_t* body, size_t bytes) {
  WindowPipe P;
  int rc = P.create(sizeof(uint64_t)); if(rc) return rc;
  const size_t win = std::min(bytes, kSortedUploadWindow);
  for(size_t o = 0, i = 0; o < bytes; o += win, ++i) {
    WindowPipe::Slot& S = P.slot[i & 1];
    const size_t len = std::min(win, bytes - o);
    if(i >= 2) HIP_TRY(hipEventSynchronize(S.up_done));
    else if((rc = S.h_in.alloc(win))) return rc;
    memcpy(S.h_in, body + o, len);
    HIP_TRY(hipMemcpyAsync(s->d_body + o, S.h_in, len, hipMemcpyHostToDevice, P.s_up));
    HIP_TRY(hipEventRecord(S.up_done, P.s_up));
  }
  HIP_TRY(hipStreamSynchronize(P.s_up));
  return JFGPU_OK;
}

}  // namespace

extern "C" {

// (no counterpart in binary_dumper.hpp:112-213: the reference maps the file and keeps no index)
int jfgpu_sorted_plan(uint64_t n_records, uint64_t size, uint32_t k, uint32_t counter_len, uint32_t records_per_bucket,
                      uint32_t* bucket_bits, uint64_t* device_bytes) {
  uint32_t lsize = 0;
  int rc = sorted_args(n_records, size, k, counter_len, &lsize); if(rc) return rc;
  const uint64_t per = records_per_bucket ? records_per_bucket : kSortedRecordsPerBucket;
  uint32_t B = 0;
  while(B < lsize && (n_records >> B) > per) ++B;
  const uint64_t kb = (2 * (uint64_t)k + 7) / 8;
  if(bucket_bits) *bucket_bits = B;
  if(device_bytes) *device_bytes = n_records * (kb + counter_len) + 32 + 8 * (((uint64_t)1 << B) + 1) + kb * 256 * 8;
  return JFGPU_OK;
}

// binary_query::binary_query (binary_dumper.hpp:112-145): the body, and here the index over it
int jfgpu_sorted_create(const jfgpu_sorted_params* p, const void* body, uint64_t n_records, jfgpu_sorted** out) {
  if(!p || !out) return fail(JFGPU_E_INVALID, "null argument");
  *out = nullptr;
  if(n_records && !body) return fail(JFGPU_E_INVALID, "sorted: null body");
  uint32_t lsize = 0, B = 0;
  int rc = sorted_args(n_records, p->size, p->k, p->counter_len, &lsize); if(rc) return rc;
  if(p->matrix_rows != lsize) return fail(JFGPU_E_INVALID, "sorted: the size (" + std::to_string(p->size) + ") is not 2^matrix_rows (2^" + std::to_string(p->matrix_rows) + ")");
  rc = jfgpu_sorted_plan(n_records, p->size, p->k, p->counter_len, p->records_per_bucket, &B, nullptr); if(rc) return rc;
  int dev = 0;
  rc = pick_device(p->device, &dev); if(rc) return rc;
  std::unique_ptr<jfgpu_sorted> s(new jfgpu_sorted);
  s->device = dev; s->k = p->k; s->key_bits = 2 * p->k; s->kb = (s->key_bits + 7) / 8; s->kw = (s->key_bits + 63) / 64;
  s->vb = p->counter_len; s->rb = s->kb + s->vb; s->size = p->size; s->lsize = lsize; s->bucket_bits = B; s->n_records = n_records;
  // the geometry the k-mers are rolled under: as the Bloom counter's, a table of the view's smallest size that is never built
  if(p->k > 64) {
    s->nword = true;
    if(!nword_geom_init(s->ng, p->k, std::max<uint32_t>(kNTileBits, nword_min_lsize(p->k)), p->canonical ? 1 : 0)) return fail(JFGPU_E_INVALID, "bad mer length");
    s->g = s->ng.g;
  } else if(p->k > 32) {
    s->wide = true;
    if(!wide_geom_init(s->wg, p->k, std::max<uint32_t>(kMaxTileBits, wide_min_lsize(p->k)), p->canonical ? 1 : 0)) return fail(JFGPU_E_INVALID, "bad mer length");
    s->g = s->wg.g;
  } else {
    const uint32_t ls = std::max<uint32_t>(std::min<uint32_t>(2 * p->k, 13), geom_min_lsize(p->k, 0));
    if(!geom_init(s->g, p->k, ls, 0, 0, p->canonical ? 1 : 0)) return fail(JFGPU_E_INVALID, "bad mer length");
  }
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  s->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  rc = s->stream.create(); if(rc) return rc;
  const size_t body_bytes = (size_t)n_records * s->rb;
  const uint64_t n_buckets = (uint64_t)1 << B;
  DevBuf<uint32_t> d_flag; DevBuf<unsigned long long> d_longest;
  if((rc = s->d_body.alloc(body_bytes + 32)) || (rc = s->d_index.alloc(n_buckets + 1)) || (rc = d_flag.alloc(1)) || (rc = d_longest.alloc(1))) return rc;
  s->device_bytes = body_bytes + 32 + 8 * (n_buckets + 1);
  if(p->matrix_columns) {
    std::vector<uint64_t> img(s->key_bits), h_fwd;
    for(uint32_t j = 0; j < s->key_bits; ++j) img[j] = p->matrix_columns[s->key_bits - 1 - j];
    gf2_byte_tables(img, s->kb, h_fwd);
    if((rc = s->d_fwd.alloc(h_fwd.size()))) return rc;
    HIP_TRY(hipMemcpy(s->d_fwd, h_fwd.data(), h_fwd.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    s->device_bytes += h_fwd.size() * sizeof(uint64_t);
  }
  HIP_TRY(hipMemsetAsync(s->d_body + body_bytes, 0, 32, s->stream));
  HIP_TRY(hipMemsetAsync(s->d_index, 0, (n_buckets + 1) * sizeof(uint64_t), s->stream));
  HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(uint32_t), s->stream));
  HIP_TRY(hipMemsetAsync(d_longest, 0, sizeof(unsigned long long), s->stream));
  auto t0 = std::chrono::steady_clock::now();
  if(body_bytes) { rc = sorted_upload(s.get(), (const uint8_t*)body, body_bytes); if(rc) return rc; }
  s->upload_us = (uint64_t)(wall_ms(t0) * 1000.0);
  t0 = std::chrono::steady_clock::now();
  uint32_t flag = 0; unsigned long long longest = 0;
  if(n_records) {
    const SortedView V = s->view();
    switch(s->kw) {
    case 1: sorted_launch_index<1>(s.get(), V, d_flag); break;
    case 2: sorted_launch_index<2>(s.get(), V, d_flag); break;
    case 3: sorted_launch_index<3>(s.get(), V, d_flag); break;
    default: sorted_launch_index<4>(s.get(), V, d_flag); break;
    }
    const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((n_buckets + kMergeBlock - 1) / kMergeBlock, (uint64_t)s->n_cu * 8));
    hipLaunchKernelGGL(sorted_longest_kernel, dim3(grid), dim3(kMergeBlock), 0, s->stream, (const uint64_t*)s->d_index, n_buckets, d_longest.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(&longest, d_longest, sizeof longest, hipMemcpyDeviceToHost, s->stream));
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->index_us = (uint64_t)(wall_ms(t0) * 1000.0);
  if(flag) return fail(JFGPU_E_INVALID, "sorted: records are not in strictly increasing (pos, key) order");
  s->longest = longest;
  *out = s.release();
  return JFGPU_OK;
}

void jfgpu_sorted_destroy(jfgpu_sorted* s) {
  if(!s) return;
  hipSetDevice(s->device);
  s->stream.sync();
  delete s;
}

int jfgpu_sorted_info(const jfgpu_sorted* s, uint64_t out6[6]) {
  if(!s || !out6) return fail(JFGPU_E_INVALID, "null argument");
  out6[0] = s->n_records; out6[1] = s->bucket_bits; out6[2] = s->longest; out6[3] = s->device_bytes; out6[4] = s->upload_us; out6[5] = s->index_us;
  return JFGPU_OK;
}

// query_from_sequence (query_main.cc:44-51) with binary_query::check (binary_dumper.hpp:191-213) over one contract buffer:
// sorted_query_ascii_kernel, the contract of jfgpu_query_ascii_dev
int jfgpu_sorted_query_ascii_dev(jfgpu_sorted* s, const char* d_bases, size_t n, uint64_t* d_vals, uint8_t* d_flags) {
  int rc = use_s(s); if(rc) return rc;
  if(!n) return JFGPU_OK;
  if(!d_bases || !d_vals) return fail(JFGPU_E_INVALID, "null argument");
  const uint8_t* base; int64_t lo, hi;
  align_buffer(d_bases, n, base, lo, hi);
  const int64_t n_tiles = (hi + kTilePos - 1) / kTilePos;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(n_tiles, (int64_t)s->n_cu * 8));
  if(s->nword) hipLaunchKernelGGL(sorted_query_ascii_kernel<NGeom>, dim3(grid), dim3(kBlock), 0, s->stream, s->view(), s->ng, base, lo, hi, d_vals, d_flags);
  else if(s->wide) hipLaunchKernelGGL(sorted_query_ascii_kernel<WideGeom>, dim3(grid), dim3(kBlock), 0, s->stream, s->view(), s->wg, base, lo, hi, d_vals, d_flags);
  else hipLaunchKernelGGL(sorted_query_ascii_kernel<TableGeom>, dim3(grid), dim3(kBlock), 0, s->stream, s->view(), s->g, base, lo, hi, d_vals, d_flags);
  HIP_TRY(hipGetLastError());
  return JFGPU_OK;
}

// Host arrays, staged like jfgpu_bc_query_ascii: pieces overlap by k - 1 bytes, and the first k - 1 outputs of every piece
// after the first (windows the piece before has answered) are not copied back.
int jfgpu_sorted_query_ascii(jfgpu_sorted* s, const char* bases, size_t n, uint64_t* vals, uint8_t* flags) {
  int rc = use_s(s); if(rc) return rc;
  if(!n) return JFGPU_OK;
  if(!bases || !vals) return fail(JFGPU_E_INVALID, "null argument");
  const size_t piece = std::min(kStageBytes, n), seam = s->k - 1;
  rc = s->d_stage.reserve(piece); if(rc) return rc;
  DevBuf<uint64_t> d_v; DevBuf<uint8_t> d_f;
  rc = d_v.alloc(piece); if(rc) return rc;
  if(flags && !d_f.try_alloc(piece)) return fail(JFGPU_E_ALLOC, "hipMalloc query flags");
  hipError_t e = hipSuccess;
  for(size_t o = 0; o < n && e == hipSuccess && !rc; o += kStageBytes - seam) {
    const size_t len = std::min(kStageBytes, n - o), skip = o ? seam : 0;
    e = hipMemcpyAsync(s->d_stage, bases + o, len, hipMemcpyHostToDevice, s->stream);
    if(e == hipSuccess) rc = jfgpu_sorted_query_ascii_dev(s, (const char*)s->d_stage.get(), len, d_v, d_f);
    if(e == hipSuccess && !rc) e = hipMemcpyAsync(vals + o + skip, d_v + skip, (len - skip) * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream);
    if(e == hipSuccess && !rc && flags) e = hipMemcpyAsync(flags + o + skip, d_f + skip, len - skip, hipMemcpyDeviceToHost, s->stream);
    if(e == hipSuccess && !rc) e = hipStreamSynchronize(s->stream);      // (the stage, d_v and d_f are the next piece's too)
    if(o + len >= n) break;
  }
  hipStreamSynchronize(s->stream);
  if(e != hipSuccess) return fail(JFGPU_E_HIP, hipGetErrorString(e));
  return rc;
}

// binary_query::check (binary_dumper.hpp:191-213) for encoded keys
int jfgpu_sorted_lookup(jfgpu_sorted* s, const uint64_t* keys, size_t n, uint64_t* vals, uint8_t* found) {
  int rc = use_s(s); if(rc) return rc;
  if(!n) return JFGPU_OK;
  if(!keys || !vals) return fail(JFGPU_E_INVALID, "null argument");
  DevBuf<uint64_t> d_k, d_v; DevBuf<uint8_t> d_f;
  rc = d_k.alloc(n * s->kw); if(rc) return rc;
  if(!d_v.try_alloc(n) || !d_f.try_alloc(n)) return fail(JFGPU_E_ALLOC, "hipMalloc lookup buffers");
  hipError_t e = hipMemcpyAsync(d_k, keys, n * sizeof(uint64_t) * s->kw, hipMemcpyHostToDevice, s->stream);
  if(e == hipSuccess) {
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((n + kBlock - 1) / kBlock, (size_t)s->n_cu * 8));
    switch(s->kw) {
    case 1: sorted_launch_lookup<1>(s, grid, d_k, n, d_v, d_f); break;
    case 2: sorted_launch_lookup<2>(s, grid, d_k, n, d_v, d_f); break;
    case 3: sorted_launch_lookup<3>(s, grid, d_k, n, d_v, d_f); break;
    default: sorted_launch_lookup<4>(s, grid, d_k, n, d_v, d_f); break;
    }
    e = hipGetLastError();
  }
  if(e == hipSuccess) e = hipMemcpyAsync(vals, d_v, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream);
  if(e == hipSuccess && found) e = hipMemcpyAsync(found, d_f, n, hipMemcpyDeviceToHost, s->stream);
  hipStreamSynchronize(s->stream);
  if(e != hipSuccess) return fail(JFGPU_E_HIP, hipGetErrorString(e));
  return JFGPU_OK;
}

// query_from_sequence (query_main.cc:44-51) with the lines built on the device, binary_query::check (binary_dumper.hpp:191-213)
// per k-mer: qtext_run answered by the records
int jfgpu_sorted_query_text(jfgpu_sorted* s, jfgpu_qtext* x, const char* bases, size_t n, jfgpu_text_sink sink, void* user) {
  int rc = use_s(s); if(rc) return rc;
  if(!x) return fail(JFGPU_E_INVALID, "null query formatter");
  rc = qtext_args(x, bases, n, sink, s->device, s->k, "sorted records"); if(rc) return rc;
  return qtext_run(x, s->stream, bases, n, sink, user,
                   [&](const char* d_bases, size_t len, uint64_t* d_vals, uint8_t* d_flags) { return jfgpu_sorted_query_ascii_dev(s, d_bases, len, d_vals, d_flags); });
}

}  // extern "C"
