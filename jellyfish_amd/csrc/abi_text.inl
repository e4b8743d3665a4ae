// jellyfish_amd/csrc/abi_text.inl -- C ABI of the device text formatter (jfgpu_text_*, jfgpu_dump_next_text), included by
// jfgpu.hip.  Kernels: kernels_text.hip.hpp.  The host side here owns the windows of jfgpu_text_run (fixed numbers of
// records, records have one width) and the two-deep pipeline of uploads, kernels and downloads, shaped as abi_merge.inl's.
struct jfgpu_text {
  int device = 0;
  TextJob job{};
  uint64_t window_records = 0;
  hipStream_t s_up = nullptr, s_k = nullptr, s_down = nullptr;
  hipEvent_t up_a[2] = {nullptr, nullptr}, up_done[2] = {nullptr, nullptr}, ev_a[2] = {nullptr, nullptr}, ev_b[2] = {nullptr, nullptr},
             k_done[2] = {nullptr, nullptr};
  uint8_t* h_in[2] = {nullptr, nullptr}; size_t h_in_cap[2] = {0, 0};     // pinned staging, in and out
  uint8_t* h_out[2] = {nullptr, nullptr}; size_t h_out_cap[2] = {0, 0};
  uint8_t* d_raw[2] = {nullptr, nullptr}; size_t raw_cap[2] = {0, 0};
  uint8_t* d_out[2] = {nullptr, nullptr}; size_t out_cap[2] = {0, 0};
  uint32_t* d_tbytes = nullptr; uint32_t* d_tkept = nullptr; uint64_t* d_toff = nullptr; size_t tile_cap = 0;
  uint64_t* d_totals = nullptr;                             // [2][2]: bytes and lines of the window in each slot
  uint64_t* h_status[2] = {nullptr, nullptr};               // pinned: the slot's two totals
  double ms[4] = {0, 0, 0, 0};                              // upload, kernels, download, sink
  uint64_t counts[4] = {0, 0, 0, 0};                        // windows, records read, records kept, bytes written
};

namespace {

int use_x(const jfgpu_text* x) {
  if(!x) return fail(JFGPU_E_INVALID, "null text formatter");
  HIP_TRY(hipSetDevice(x->device));
  return JFGPU_OK;
}

int text_grow_tiles(jfgpu_text* x, size_t nb) {
  if(nb <= x->tile_cap) return JFGPU_OK;
  HIP_TRY(hipStreamSynchronize(x->s_k));
  for(void* p : {(void*)x->d_tbytes, (void*)x->d_tkept, (void*)x->d_toff}) if(p) HIP_TRY(hipFree(p));
  x->d_tbytes = x->d_tkept = nullptr; x->d_toff = nullptr; x->tile_cap = 0;
  const size_t cap = nb + nb / 8 + 16;
  HIP_TRY(hipMalloc((void**)&x->d_tbytes, cap * sizeof(uint32_t)));
  HIP_TRY(hipMalloc((void**)&x->d_tkept, cap * sizeof(uint32_t)));
  HIP_TRY(hipMalloc((void**)&x->d_toff, cap * sizeof(uint64_t)));
  x->tile_cap = cap;
  return JFGPU_OK;
}

// The three launches for n > 0 records at d_rec, on s_k; the totals go to d_totals[2 * slot ..].  text_write_kernel writes
// nothing when the text is longer than cap_bytes.  The tile arrays hold (n + 255) / 256 entries (text_grow_tiles).
void text_launch(jfgpu_text* x, const uint8_t* d_rec, uint64_t n, uint8_t* d_text, uint64_t cap_bytes, int slot) {
  const uint32_t nb = (uint32_t)((n + kTextBlock - 1) / kTextBlock);
  const uint32_t lds_raw = text_lds_raw(x->job.rb), lds_out = text_lds_out(x->job.line_max);
  hipLaunchKernelGGL(text_len_kernel, dim3(nb), dim3(kTextBlock), lds_raw, x->s_k, x->job, d_rec, n, x->d_tbytes, x->d_tkept);
  hipLaunchKernelGGL(text_scan_kernel, dim3(1), dim3(kTextBlock), 0, x->s_k, (const uint32_t*)x->d_tbytes, (const uint32_t*)x->d_tkept, nb, x->d_toff,
                     x->d_totals + 2 * slot);
  hipLaunchKernelGGL(text_write_kernel, dim3(nb), dim3(kTextBlock), lds_raw + lds_out, x->s_k, x->job, d_rec, n, (const uint64_t*)x->d_toff,
                     (const uint64_t*)(x->d_totals + 2 * slot), cap_bytes, d_text);
}

constexpr uint64_t kTextMaxRecords = (uint64_t)1 << 31;      // of one window / one format_dev call: tiles are a 32-bit grid

}  // namespace

extern "C" {

int jfgpu_text_create(const jfgpu_text_params* p, jfgpu_text** out) {
  if(!p || !out) return fail(JFGPU_E_INVALID, "null argument");
  *out = nullptr;
  if(p->k < 1 || p->k > 128) return fail(JFGPU_E_UNSUPPORTED, "text: mer length must be in [1, 128]");
  if(p->counter_len < 1 || p->counter_len > 8) return fail(JFGPU_E_INVALID, "text: counter_len must be in [1, 8]");
  if(p->layout != JFGPU_TEXT_COLUMN && p->layout != JFGPU_TEXT_FASTA) return fail(JFGPU_E_INVALID, "text: layout must be 0 column or 1 FASTA");
  if(p->layout == JFGPU_TEXT_COLUMN && p->separator != ' ' && p->separator != '\t') return fail(JFGPU_E_INVALID, "text: the separator must be a space or a tab");
  if(p->window_records > kTextMaxRecords) return fail(JFGPU_E_INVALID, "text: window_records must be at most 2^31");
  int ndev = 0;
  if(hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(JFGPU_E_NO_DEVICE, "no HIP device: the engine has no CPU fallback");
  int dev = p->device;
  if(dev < 0) HIP_TRY(hipGetDevice(&dev));
  if(dev >= ndev) return fail(JFGPU_E_NO_DEVICE, "device ordinal out of range");
  HIP_TRY(hipSetDevice(dev));
  std::unique_ptr<jfgpu_text, void (*)(jfgpu_text*)> x(new jfgpu_text, jfgpu_text_destroy);
  x->device = dev;
  TextJob& J = x->job;
  J.k = p->k; J.kb = (2 * p->k + 7) / 8; J.vb = p->counter_len; J.rb = J.kb + J.vb;
  J.layout = p->layout; J.sep = p->layout == JFGPU_TEXT_COLUMN ? p->separator : (uint32_t)' '; J.pad_ = 0;
  J.lower = p->lower; J.upper = p->upper;
  const uint64_t vmax = J.vb >= 8 ? ~0ull : ((1ull << (8 * J.vb)) - 1);
  J.line_max = J.k + 2 + text_digits(std::min(vmax, p->upper)) + (J.layout == kTextFasta ? 1 : 0);
  x->window_records = p->window_records ? p->window_records : kTextWindowRecords;
  HIP_TRY(hipStreamCreateWithFlags(&x->s_up, hipStreamNonBlocking));
  HIP_TRY(hipStreamCreateWithFlags(&x->s_k, hipStreamNonBlocking));
  HIP_TRY(hipStreamCreateWithFlags(&x->s_down, hipStreamNonBlocking));
  for(int i = 0; i < 2; ++i) {
    HIP_TRY(hipEventCreate(&x->up_a[i])); HIP_TRY(hipEventCreate(&x->up_done[i]));
    HIP_TRY(hipEventCreate(&x->ev_a[i])); HIP_TRY(hipEventCreate(&x->ev_b[i])); HIP_TRY(hipEventCreate(&x->k_done[i]));
    HIP_TRY(hipHostMalloc((void**)&x->h_status[i], 2 * sizeof(uint64_t), hipHostMallocDefault));
  }
  HIP_TRY(hipMalloc((void**)&x->d_totals, 4 * sizeof(uint64_t)));
  *out = x.release();
  return JFGPU_OK;
}

void jfgpu_text_destroy(jfgpu_text* x) {
  if(!x) return;
  hipSetDevice(x->device);
  for(hipStream_t s : {x->s_up, x->s_k, x->s_down}) if(s) { hipStreamSynchronize(s); hipStreamDestroy(s); }
  for(int i = 0; i < 2; ++i) {
    for(hipEvent_t e : {x->up_a[i], x->up_done[i], x->ev_a[i], x->ev_b[i], x->k_done[i]}) if(e) hipEventDestroy(e);
    if(x->h_in[i]) hipHostFree(x->h_in[i]);
    if(x->h_out[i]) hipHostFree(x->h_out[i]);
    if(x->h_status[i]) hipHostFree(x->h_status[i]);
    hipFree(x->d_raw[i]); hipFree(x->d_out[i]);
  }
  hipFree(x->d_tbytes); hipFree(x->d_tkept); hipFree(x->d_toff); hipFree(x->d_totals);
  delete x;
}

int jfgpu_text_line_max(const jfgpu_text* x, uint32_t* bytes) {
  if(!x || !bytes) return fail(JFGPU_E_INVALID, "null argument");
  *bytes = x->job.line_max;
  return JFGPU_OK;
}

int jfgpu_text_run(jfgpu_text* x, const void* body, uint64_t n_records, jfgpu_text_sink sink, void* user) {
  int rc = use_x(x); if(rc) return rc;
  if(!sink) return fail(JFGPU_E_INVALID, "text: no sink");
  if(n_records && !body) return fail(JFGPU_E_INVALID, "text: null body");
  HIP_TRY(hipStreamSynchronize(x->s_up)); HIP_TRY(hipStreamSynchronize(x->s_k)); HIP_TRY(hipStreamSynchronize(x->s_down));   // (a run that failed may have left work behind)
  for(int i = 0; i < 4; ++i) { x->ms[i] = 0; x->counts[i] = 0; }
  const uint32_t rb = x->job.rb, line_max = x->job.line_max;
  const uint64_t W = x->window_records;
  const uint64_t n_win = (n_records + W - 1) / W;
  auto win_n = [&](uint64_t i) { return std::min<uint64_t>(W, n_records - i * W); };
  if(n_win) {
    // every buffer at the size of the largest window, once: nothing grows while the pipeline runs
    const uint64_t wmax = win_n(0);
    rc = text_grow_tiles(x, (size_t)((wmax + kTextBlock - 1) / kTextBlock)); if(rc) return rc;
    for(int s = 0; s < (n_win > 1 ? 2 : 1); ++s) {
      rc = grow_buf(x->d_raw[s], x->raw_cap[s], (size_t)wmax * rb + 64); if(rc) return rc;       // (read to the next 16-byte boundary)
      rc = grow_buf(x->d_out[s], x->out_cap[s], (size_t)wmax * line_max + 64); if(rc) return rc;
      rc = merge_grow_host(x->h_in[s], x->h_in_cap[s], (size_t)wmax * rb); if(rc) return rc;
    }
  }

  // the download and the sink of a window whose kernels are enqueued
  auto finish = [&](uint64_t j) -> int {
    const int slot = (int)(j & 1);
    HIP_TRY(hipEventSynchronize(x->k_done[slot]));
    float ms = 0;
    if(hipEventElapsedTime(&ms, x->ev_a[slot], x->ev_b[slot]) == hipSuccess) x->ms[1] += ms;
    if(hipEventElapsedTime(&ms, x->up_a[slot], x->up_done[slot]) == hipSuccess) x->ms[0] += ms;
    const uint64_t nbytes = x->h_status[slot][0], nkept = x->h_status[slot][1];
    if(nkept > win_n(j) || nbytes > nkept * line_max) return fail(JFGPU_E_HIP, "text: the device wrote more than the window can hold");
    x->counts[2] += nkept; x->counts[3] += nbytes;
    if(nbytes) {
      auto t0 = std::chrono::steady_clock::now();
      rc = merge_grow_host(x->h_out[slot], x->h_out_cap[slot], (size_t)nbytes); if(rc) return rc;
      HIP_TRY(hipMemcpyAsync(x->h_out[slot], x->d_out[slot], (size_t)nbytes, hipMemcpyDeviceToHost, x->s_down));
      HIP_TRY(hipStreamSynchronize(x->s_down));
      x->ms[2] += merge_wall_ms(t0);
      t0 = std::chrono::steady_clock::now();
      if(sink(user, (const char*)x->h_out[slot], nbytes, nkept)) return fail(JFGPU_E_INVALID, "text: the sink asked to stop");
      x->ms[3] += merge_wall_ms(t0);
    }
    return JFGPU_OK;
  };

  bool pending = false;
  for(uint64_t i = 0; i < n_win; ++i) {
    const int slot = (int)(i & 1);
    const uint64_t n = win_n(i);
    // ---- stage and upload (the kernels of window i - 1 run meanwhile)
    auto t0 = std::chrono::steady_clock::now();
    memcpy(x->h_in[slot], (const uint8_t*)body + i * W * rb, (size_t)n * rb);
    x->ms[0] += merge_wall_ms(t0);
    HIP_TRY(hipEventRecord(x->up_a[slot], x->s_up));
    HIP_TRY(hipMemcpyAsync(x->d_raw[slot], x->h_in[slot], (size_t)n * rb, hipMemcpyHostToDevice, x->s_up));
    HIP_TRY(hipEventRecord(x->up_done[slot], x->s_up));
    // ---- kernels
    HIP_TRY(hipStreamWaitEvent(x->s_k, x->up_done[slot], 0));
    HIP_TRY(hipEventRecord(x->ev_a[slot], x->s_k));
    text_launch(x, x->d_raw[slot], n, x->d_out[slot], n * line_max, slot);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(x->ev_b[slot], x->s_k));
    HIP_TRY(hipMemcpyAsync(x->h_status[slot], x->d_totals + 2 * slot, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, x->s_k));
    HIP_TRY(hipEventRecord(x->k_done[slot], x->s_k));
    x->counts[0] += 1; x->counts[1] += n;
    // ---- the window before this one: download and sink while this one's kernels run
    if(pending) { pending = false; rc = finish(i - 1); if(rc) { hipStreamSynchronize(x->s_k); return rc; } }
    pending = true;
  }
  if(pending) { rc = finish(n_win - 1); if(rc) return rc; }
  return JFGPU_OK;
}

int jfgpu_text_format_dev(jfgpu_text* x, const void* d_records, uint64_t n_records, char* d_text, uint64_t capacity_bytes,
                          uint64_t* n_bytes, uint64_t* n_kept) {
  int rc = use_x(x); if(rc) return rc;
  if(!n_bytes || !n_kept) return fail(JFGPU_E_INVALID, "null argument");
  *n_bytes = *n_kept = 0;
  if(n_records == 0) return JFGPU_OK;
  if(!d_records || (!d_text && capacity_bytes)) return fail(JFGPU_E_INVALID, "null argument");
  if((uintptr_t)d_records & 15u) return fail(JFGPU_E_INVALID, "text: the records must start on a 16-byte boundary");
  if(n_records > kTextMaxRecords) return fail(JFGPU_E_UNSUPPORTED, "text: at most 2^31 records a call");
  HIP_TRY(hipStreamSynchronize(x->s_k));
  rc = text_grow_tiles(x, (size_t)((n_records + kTextBlock - 1) / kTextBlock)); if(rc) return rc;
  text_launch(x, (const uint8_t*)d_records, n_records, (uint8_t*)d_text, capacity_bytes, 0);
  HIP_TRY(hipGetLastError());
  uint64_t tot[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(tot, x->d_totals, sizeof tot, hipMemcpyDeviceToHost, x->s_k));
  HIP_TRY(hipStreamSynchronize(x->s_k));
  *n_bytes = tot[0]; *n_kept = tot[1];
  if(tot[0] > capacity_bytes)
    return fail(JFGPU_E_INVALID, "text: the output needs " + std::to_string(tot[0]) + " bytes, the buffer holds " + std::to_string(capacity_bytes) + " (nothing was written)");
  return JFGPU_OK;
}

int jfgpu_text_last_ms(jfgpu_text* x, double out4[4]) {
  if(!x || !out4) return fail(JFGPU_E_INVALID, "null argument");
  for(int i = 0; i < 4; ++i) out4[i] = x->ms[i];
  return JFGPU_OK;
}

int jfgpu_text_counts(jfgpu_text* x, uint64_t out4[4]) {
  if(!x || !out4) return fail(JFGPU_E_INVALID, "null argument");
  for(int i = 0; i < 4; ++i) out4[i] = x->counts[i];
  return JFGPU_OK;
}

int jfgpu_dump_next_text(jfgpu_table* t, jfgpu_text* x, char* out, uint64_t capacity_bytes, uint64_t* n_records, uint64_t* n_bytes) {
  int rc = use(t); if(rc) return rc;
  if(!x || !out || !n_records || !n_bytes) return fail(JFGPU_E_INVALID, "null argument");
  *n_records = *n_bytes = 0;
  if(!t->dump_open) return fail(JFGPU_E_INVALID, "jfgpu_dump_begin not called");
  if(x->device != t->device) return fail(JFGPU_E_INVALID, "dump_next_text: the formatter lives on another device than the table");
  if(x->job.k != t->params.k || x->job.vb != t->out_counter_len)
    return fail(JFGPU_E_INVALID, "dump_next_text: the formatter's k and counter_len (" + std::to_string(x->job.k) + ", " + std::to_string(x->job.vb) +
                ") are not the table's (" + std::to_string(t->params.k) + ", " + std::to_string(t->out_counter_len) + ")");
  const uint64_t tsz = 1ull << t->g.tile_bits;
  const uint64_t cap_rec = std::min<uint64_t>(capacity_bytes / x->job.line_max, kTextMaxRecords);
  if(cap_rec < tsz)
    return fail(JFGPU_E_INVALID, "dump_next_text: the buffer must hold the text of one tile (" + std::to_string(tsz * x->job.line_max) + " bytes)");
  HIP_TRY(hipStreamSynchronize(x->s_k));
  const uint64_t cursor = t->dump_tile_cursor;
  uint64_t nrec = 0;
  rc = dump_next_chunk(t, cap_rec, &nrec); if(rc) return rc;
  if(!nrec) return JFGPU_OK;
  // a failure from here on leaves the chunk undelivered: the cursor goes back, the next call produces it again
  auto undo = [&](int code) { t->dump_tile_cursor = cursor; hipStreamSynchronize(t->stream); return code; };
  if((rc = text_grow_tiles(x, (size_t)((nrec + kTextBlock - 1) / kTextBlock))) || (rc = grow_buf(x->d_out[0], x->out_cap[0], (size_t)nrec * x->job.line_max + 64)))
    return undo(rc);
  hipError_t e = hipStreamSynchronize(t->stream);                  // the chunk is in d_dump
  uint64_t tot[2] = {0, 0};
  if(e == hipSuccess) {
    text_launch(x, t->d_dump, nrec, x->d_out[0], nrec * x->job.line_max, 0);
    e = hipGetLastError();
  }
  if(e == hipSuccess) e = hipMemcpyAsync(tot, x->d_totals, sizeof tot, hipMemcpyDeviceToHost, x->s_k);
  if(e == hipSuccess) e = hipStreamSynchronize(x->s_k);
  if(e == hipSuccess && (tot[1] > nrec || tot[0] > capacity_bytes))
    return undo(fail(JFGPU_E_HIP, "dump_next_text: the device wrote more than the chunk can hold"));
  if(e == hipSuccess && tot[0]) e = hipMemcpyAsync(out, x->d_out[0], tot[0], hipMemcpyDeviceToHost, x->s_k);
  if(e == hipSuccess) e = hipStreamSynchronize(x->s_k);
  if(e != hipSuccess) return undo(fail(JFGPU_E_HIP, hipGetErrorString(e)));
  *n_records = nrec; *n_bytes = tot[0];
  return JFGPU_OK;
}

}  // extern "C"
