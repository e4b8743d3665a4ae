// jellyfish_amd/csrc/abi_merge.inl -- C ABI of the device merge of sorted databases (jfgpu_merge_*), included by jfgpu.hip.
// Kernels: kernels_merge.hip.hpp.  The host side here owns the windowing (cuts of every input at position boundaries,
// found by binary search over the caller's mapped bodies), the two-deep pipeline of uploads, kernels and downloads, and
// the growth of the working buffers when one position holds more than a window.  The pipeline's streams, events and
// per-slot buffers are a WindowPipe (hip_own.hpp), shared with abi_text.inl; what is the merge's own is here.
struct jfgpu_merge {
  int device = 0;
  WindowPipe pipe;                                          // (first: its streams outlive the buffers below)
  uint32_t k = 0, kb = 0, kw = 0, key_bits = 0, n_inputs = 0, ocl = 0;
  int op = 0;
  uint64_t size = 0, lower = 0, upper = 0, window_records = 0, vmax = 0;
  bool identity = false;
  std::vector<uint32_t> clen;
  std::vector<uint64_t> h_fwd;                              // byte tables of the matrix, for the host's cuts too
  DevBuf<uint64_t> d_fwd;
  DevBuf<uint64_t> d_keys, d_vals, d_pos, d_oval, d_boff; DevBuf<uint32_t> d_osrc, d_bcnt; size_t rec_cap = 0;    // of one window's records
  DevBuf<uint64_t> d_nkept;                                 // [2]
  DevBuf<uint32_t> d_unsorted;                              // [n_inputs]
  DevBuf<unsigned long long> d_tallies;                     // [4]
  uint64_t tallies[4] = {0, 0, 0, 0};                       // (a slot's status block: n_kept, then the unsorted flags)
  uint64_t counts[3] = {0, 0, 0};                           // windows, records in, records out
};

namespace {

struct MergeWindow { std::vector<uint64_t> lo, hi; uint64_t total = 0; };

int use_m(const jfgpu_merge* m) { return use_dev(m, "null merge"); }

// pos of the record at rec: the kernels' product, byte table by byte table
uint64_t merge_host_pos(const jfgpu_merge* m, const uint8_t* rec) {
  const uint32_t top = m->key_bits - 8 * (m->kb - 1);       // bits of the key in its last byte
  const uint8_t last = (uint8_t)(rec[m->kb - 1] & ((1u << top) - 1u));
  uint64_t p = 0;
  if(m->identity) {
    for(uint32_t b = 0; b < m->kb && b < 8; ++b) p |= (uint64_t)(b == m->kb - 1 ? last : rec[b]) << (8 * b);
  } else {
    for(uint32_t b = 0; b + 1 < m->kb; ++b) p ^= m->h_fwd[(size_t)b * 256 + rec[b]];
    p ^= m->h_fwd[(size_t)(m->kb - 1) * 256 + last];
  }
  return p & (m->size - 1);
}

// first record of input f in [lo, hi) whose pos is not below P
uint64_t merge_cut(const jfgpu_merge* m, const uint8_t* body, uint32_t rb, uint64_t lo, uint64_t hi, uint64_t P) {
  while(lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if(merge_host_pos(m, body + mid * rb) < P) lo = mid + 1; else hi = mid;
  }
  return lo;
}

void merge_split(const jfgpu_merge* m, const void* const* bodies, uint64_t P0, uint64_t P1, const std::vector<uint64_t>& lo,
                 const std::vector<uint64_t>& hi, std::vector<MergeWindow>& out) {
  uint64_t total = 0;
  for(uint32_t f = 0; f < m->n_inputs; ++f) total += hi[f] - lo[f];
  if(total == 0) return;
  if(total <= m->window_records || P1 - P0 <= 1) { MergeWindow w; w.lo = lo; w.hi = hi; w.total = total; out.push_back(std::move(w)); return; }
  const uint64_t mid = P0 + ((P1 - P0) >> 1);
  std::vector<uint64_t> cut(m->n_inputs);
  for(uint32_t f = 0; f < m->n_inputs; ++f) cut[f] = merge_cut(m, (const uint8_t*)bodies[f], m->kb + m->clen[f], lo[f], hi[f], mid);
  merge_split(m, bodies, P0, mid, lo, cut, out);
  merge_split(m, bodies, mid, P1, cut, hi, out);
}

size_t merge_segs_bytes(const jfgpu_merge* m) { return ((size_t)m->n_inputs * sizeof(MergeSeg) + 255) & ~(size_t)255; }

template <int KW>
void merge_launch(jfgpu_merge* m, const MergeWin& W, const uint8_t* raw, int slot) {
  const uint64_t pos_mask = m->size - 1;
  const hipStream_t s_k = m->pipe.s_k;
  hipLaunchKernelGGL((merge_decode_kernel<KW>), dim3(W.n_tiles), dim3(kMergeBlock), 0, s_k, W, raw,
                     (const uint64_t*)(m->identity ? nullptr : m->d_fwd.get()), m->kb, m->key_bits, pos_mask, m->d_unsorted.get());
  hipLaunchKernelGGL((merge_rank_kernel<KW>), dim3(W.n_tiles), dim3(kMergeBlock), 0, s_k, W, m->op, m->lower, m->upper, m->vmax,
                     m->d_oval.get(), m->d_osrc.get(), m->d_tallies.get());
  if(m->op == 3) return;
  const uint32_t nb = (uint32_t)((W.total + kMergeBlock - 1) / kMergeBlock);
  hipLaunchKernelGGL(merge_count_kernel, dim3(nb), dim3(kMergeBlock), 0, s_k, (const uint32_t*)m->d_osrc, W.total, m->d_bcnt.get());
  hipLaunchKernelGGL(merge_scan_kernel, dim3(1), dim3(kMergeBlock), 0, s_k, (const uint32_t*)m->d_bcnt, nb, m->d_boff.get(), m->d_nkept + slot);
  hipLaunchKernelGGL((merge_pack_kernel<KW>), dim3(nb), dim3(kMergeBlock), 0, s_k, W, (const uint64_t*)m->d_oval, (const uint32_t*)m->d_osrc,
                     (const uint64_t*)m->d_boff, m->kb, m->ocl, m->pipe.slot[slot].d_out.get());
}

}  // namespace

extern "C" {

int jfgpu_merge_create(const jfgpu_merge_params* p, jfgpu_merge** out) {
  if(!p || !out) return fail(JFGPU_E_INVALID, "null argument");
  *out = nullptr;
  if(p->k < 1 || p->k > 128) return fail(JFGPU_E_UNSUPPORTED, "merge: mer length must be in [1, 128]");
  if(p->n_inputs < 1 || p->n_inputs > kMergeMaxInputs) return fail(JFGPU_E_UNSUPPORTED, "merge: the device path takes 1 to " + std::to_string(kMergeMaxInputs) + " inputs");
  if(p->size == 0 || (p->size & (p->size - 1))) return fail(JFGPU_E_INVALID, "merge: size must be a power of two");
  if(!p->counter_len) return fail(JFGPU_E_INVALID, "merge: null counter_len");
  if(p->out_counter_len < 1 || p->out_counter_len > 8) return fail(JFGPU_E_INVALID, "merge: out_counter_len must be in [1, 8]");
  if(p->op > 3) return fail(JFGPU_E_INVALID, "merge: operation must be 0 sum, 1 min, 2 max or 3 Jaccard");
  for(uint32_t f = 0; f < p->n_inputs; ++f)
    if(p->counter_len[f] < 1 || p->counter_len[f] > 8) return fail(JFGPU_E_INVALID, "merge: counter_len must be in [1, 8]");
  int dev = 0;
  int rc = pick_device(p->device, &dev); if(rc) return rc;
  std::unique_ptr<jfgpu_merge> m(new jfgpu_merge);
  m->device = dev; m->k = p->k; m->key_bits = 2 * p->k; m->kb = (m->key_bits + 7) / 8; m->kw = (m->key_bits + 63) / 64;
  m->n_inputs = p->n_inputs; m->ocl = p->out_counter_len; m->op = (int)p->op; m->size = p->size; m->lower = p->lower; m->upper = p->upper;
  m->window_records = p->window_records ? p->window_records : kMergeWindowRecords;
  m->vmax = m->ocl >= 8 ? ~0ull : ((1ull << (8 * m->ocl)) - 1);
  m->clen.assign(p->counter_len, p->counter_len + p->n_inputs);
  m->identity = p->matrix_columns == nullptr;
  if(!m->identity) {
    std::vector<uint64_t> img(m->key_bits);
    for(uint32_t j = 0; j < m->key_bits; ++j) img[j] = p->matrix_columns[m->key_bits - 1 - j];
    gf2_byte_tables(img, m->kb, m->h_fwd);
    if((rc = m->d_fwd.alloc(m->h_fwd.size()))) return rc;
    HIP_TRY(hipMemcpy(m->d_fwd, m->h_fwd.data(), m->h_fwd.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  }
  if((rc = m->pipe.create(8 + 4 * (size_t)m->n_inputs)) || (rc = m->d_nkept.alloc(2)) || (rc = m->d_unsorted.alloc(m->n_inputs)) || (rc = m->d_tallies.alloc(4))) return rc;
  *out = m.release();
  return JFGPU_OK;
}

void jfgpu_merge_destroy(jfgpu_merge* m) {
  if(!m) return;
  hipSetDevice(m->device);
  m->pipe.sync();
  delete m;
}

int jfgpu_merge_run(jfgpu_merge* m, const void* const* bodies, const uint64_t* n_records, jfgpu_merge_sink sink, void* user) {
  int rc = use_m(m); if(rc) return rc;
  if(!bodies || !n_records) return fail(JFGPU_E_INVALID, "null argument");
  if(m->op != 3 && !sink) return fail(JFGPU_E_INVALID, "merge: no sink");
  for(uint32_t f = 0; f < m->n_inputs; ++f) if(n_records[f] && !bodies[f]) return fail(JFGPU_E_INVALID, "merge: null body");
  WindowPipe& P = m->pipe;
  rc = P.begin_run(); if(rc) return rc;
  for(int i = 0; i < 4; ++i) m->tallies[i] = 0;
  m->counts[0] = m->counts[1] = m->counts[2] = 0;
  const uint32_t nf = m->n_inputs, orb = m->kb + m->ocl;

  // ---- windows: equal slices of the position range, halved while they hold more than window_records
  std::vector<MergeWindow> wins;
  {
    uint64_t total = 0;
    for(uint32_t f = 0; f < nf; ++f) total += n_records[f];
    uint64_t slices = std::max<uint64_t>(1, (total + m->window_records - 1) / m->window_records);
    slices = std::min<uint64_t>(std::min<uint64_t>(slices, m->size), (uint64_t)1 << 20);
    std::vector<uint64_t> lo(nf, 0), hi(nf);
    uint64_t P0 = 0;
    for(uint64_t j = 1; j <= slices; ++j) {
      const uint64_t P1 = j == slices ? m->size : (uint64_t)(((unsigned __int128)m->size * j) / slices);
      for(uint32_t f = 0; f < nf; ++f)
        hi[f] = j == slices ? n_records[f] : merge_cut(m, (const uint8_t*)bodies[f], m->kb + m->clen[f], lo[f], n_records[f], P1);
      merge_split(m, bodies, P0, P1, lo, hi, wins);
      lo = hi; P0 = P1;
    }
  }

  HIP_TRY(hipMemsetAsync(m->d_unsorted, 0, nf * sizeof(uint32_t), P.s_k));
  HIP_TRY(hipMemsetAsync(m->d_tallies, 0, 4 * sizeof(unsigned long long), P.s_k));

  const size_t segs_bytes = merge_segs_bytes(m);
  bool sunk = false;
  // the download, the check and the sink of a window whose kernels are enqueued
  auto finish = [&](size_t j) -> int {
    const int slot = (int)(j & 1);
    int frc = P.wait(slot); if(frc) return frc;
    const uint64_t* status = P.status_words(slot);
    const uint32_t* flags = (const uint32_t*)(status + 1);
    for(uint32_t f = 0; f < nf; ++f)
      if(flags[f]) return fail(JFGPU_E_FORMAT, "merge: input " + std::to_string(f) + " is not sorted by (position, key)" + (sunk ? " (output already written)" : ""));
    const uint64_t nk = m->op == 3 ? 0 : status[0];
    if(nk > wins[j].total) return fail(JFGPU_E_HIP, "merge: the device kept more records than the window holds");
    m->counts[2] += nk;
    if(nk) {
      frc = P.download(slot, (size_t)nk * orb); if(frc) return frc;
      sunk = true;
      if(P.sink([&] { return sink(user, P.slot[slot].h_out, nk); })) return fail(JFGPU_E_INVALID, "merge: the sink asked to stop");
    }
    return JFGPU_OK;
  };

  long pending = -1;
  for(size_t i = 0; i < wins.size(); ++i) {
    const MergeWindow& w = wins[i];
    const int slot = (int)(i & 1);
    WindowPipe::Slot& S = P.slot[slot];
    if(w.total >= ((uint64_t)1 << 31)) return fail(JFGPU_E_UNSUPPORTED, "merge: one position holds 2^31 records or more");
    // ---- layout of the window's bytes: the segment table, then every input's records from a 16-byte boundary
    size_t in_bytes = segs_bytes;
    uint32_t n_tiles = 0;
    std::vector<MergeSeg> segs(nf);
    uint64_t first = 0;
    for(uint32_t f = 0; f < nf; ++f) {
      MergeSeg& s = segs[f];
      s.raw_off = in_bytes - segs_bytes; s.first = first; s.n = w.hi[f] - w.lo[f]; s.tile0 = n_tiles;
      s.rb = m->kb + m->clen[f]; s.counter_len = m->clen[f]; s.pad_ = 0;
      in_bytes += ((size_t)s.n * s.rb + 15) & ~(size_t)15;
      first += s.n;
      n_tiles += (uint32_t)((s.n + kMergeBlock - 1) / kMergeBlock);
    }
    const size_t raw_need = in_bytes + 64;                   // the decode reads up to 32 bytes past the last record
    const size_t out_need = (size_t)w.total * orb + 64;
    if(w.total > m->rec_cap || raw_need > S.d_raw.cap() || out_need > S.d_out.cap()) {
      // one position holds more than a window, or the first windows: everything in flight ends, then the buffers grow
      if(pending >= 0) { rc = finish((size_t)pending); pending = -1; if(rc) return rc; }
      HIP_TRY(hipStreamSynchronize(P.s_up)); HIP_TRY(hipStreamSynchronize(P.s_k));
      if((rc = S.d_raw.reserve(raw_need)) || (rc = S.d_out.reserve(out_need))) return rc;
      if(w.total > m->rec_cap) {
        const size_t cap = (size_t)w.total + (size_t)w.total / 8, nb = cap / kMergeBlock + 2;
        m->rec_cap = 0;
        if((rc = m->d_keys.alloc(cap * m->kw)) || (rc = m->d_vals.alloc(cap)) || (rc = m->d_pos.alloc(cap)) || (rc = m->d_oval.alloc(cap)) ||
           (rc = m->d_osrc.alloc(cap)) || (rc = m->d_bcnt.alloc(nb)) || (rc = m->d_boff.alloc(nb))) return rc;
        m->rec_cap = cap;
      }
    }
    // ---- stage and upload (the kernels of window i - 1 run meanwhile)
    const auto t0 = std::chrono::steady_clock::now();
    rc = S.h_in.reserve(in_bytes); if(rc) return rc;
    memcpy(S.h_in, segs.data(), nf * sizeof(MergeSeg));
    for(uint32_t f = 0; f < nf; ++f)
      if(segs[f].n) memcpy(S.h_in + segs_bytes + segs[f].raw_off, (const uint8_t*)bodies[f] + w.lo[f] * segs[f].rb, (size_t)segs[f].n * segs[f].rb);
    rc = P.upload(slot, in_bytes, t0); if(rc) return rc;
    // ---- kernels
    MergeWin W;
    W.segs = (const MergeSeg*)S.d_raw.get(); W.n_inputs = nf; W.n_tiles = n_tiles; W.total = w.total; W.cap = m->rec_cap;
    W.keys = m->d_keys; W.vals = m->d_vals; W.pos = m->d_pos;
    rc = P.kernels_begin(slot); if(rc) return rc;
    const uint8_t* raw = S.d_raw + segs_bytes;                 // the records follow the segment table in the same buffer
    switch(m->kw) {
    case 1: merge_launch<1>(m, W, raw, slot); break;
    case 2: merge_launch<2>(m, W, raw, slot); break;
    case 3: merge_launch<3>(m, W, raw, slot); break;
    default: merge_launch<4>(m, W, raw, slot); break;
    }
    rc = P.kernels_end(slot); if(rc) return rc;
    if(m->op != 3) { rc = P.status(slot, 0, m->d_nkept + slot, sizeof(uint64_t)); if(rc) return rc; }
    if((rc = P.status(slot, 1, m->d_unsorted, nf * sizeof(uint32_t))) || (rc = P.done(slot))) return rc;
    m->counts[0] += 1; m->counts[1] += w.total;
    // ---- the window before this one: download and sink while this one's kernels run
    if(pending >= 0) { rc = finish((size_t)pending); pending = -1; if(rc) { hipStreamSynchronize(P.s_k); return rc; } }
    pending = (long)i;
  }
  if(pending >= 0) { rc = finish((size_t)pending); if(rc) return rc; }
  if(m->op == 3) {
    HIP_TRY(hipMemcpyAsync(m->tallies, m->d_tallies, sizeof m->tallies, hipMemcpyDeviceToHost, P.s_k));
    HIP_TRY(hipStreamSynchronize(P.s_k));
  }
  return JFGPU_OK;
}

int jfgpu_merge_tallies(jfgpu_merge* m, uint64_t out4[4]) {
  if(!m || !out4) return fail(JFGPU_E_INVALID, "null argument");
  for(int i = 0; i < 4; ++i) out4[i] = m->tallies[i];
  return JFGPU_OK;
}

int jfgpu_merge_last_ms(jfgpu_merge* m, double out4[4]) {
  if(!m || !out4) return fail(JFGPU_E_INVALID, "null argument");
  for(int i = 0; i < 4; ++i) out4[i] = m->pipe.ms[i];
  return JFGPU_OK;
}

int jfgpu_merge_counts(jfgpu_merge* m, uint64_t out3[3]) {
  if(!m || !out3) return fail(JFGPU_E_INVALID, "null argument");
  for(int i = 0; i < 3; ++i) out3[i] = m->counts[i];
  return JFGPU_OK;
}

}  // extern "C"
