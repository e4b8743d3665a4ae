// jellyfish_amd/csrc/abi_qtext.inl -- C ABI of the device formatter of `query -s` (jfgpu_qtext_*, jfgpu_query_text,
// jfgpu_bc_query_text), included by jfgpu.hip.  Kernels: kernels_qtext.hip.hpp and text_scan_kernel.  The host forms cut a
// host buffer into pieces that overlap by k - 1 bytes and move them through a WindowPipe (hip_own.hpp), the pipeline under
// abi_text.inl and abi_merge.inl: a slot holds a piece's bases, its answer (vals and flags) and its text.  The look-up runs
// on the stream of whoever answers (the table's or the Bloom counter's), between the slot's upload and its format kernels.
struct jfgpu_qtext {
  int device = 0;
  WindowPipe pipe;                                          // (first: its streams outlive the buffers below)
  QTextJob job{};
  uint64_t piece_positions = 0;
  DevBuf<uint32_t> d_tbytes, d_tkept; DevBuf<uint64_t> d_toff; size_t tile_cap = 0;
  DevBuf<uint64_t> d_totals;                                // [2][2]: bytes and lines of the piece in each slot
  DevBuf<uint64_t> d_vals[2]; DevBuf<uint8_t> d_flags[2];   // a slot's answer
  Event asked[2];                                           // the slot's look-up has been enqueued on the answerer's stream
  uint64_t counts[4] = {0, 0, 0, 0};                        // pieces, positions, lines, bytes
};

namespace {

int use_q(const jfgpu_qtext* x) { return use_dev(x, "null query formatter"); }

int qtext_grow_tiles(jfgpu_qtext* x, size_t nb) {
  if(nb <= x->tile_cap) return JFGPU_OK;
  HIP_TRY(hipStreamSynchronize(x->pipe.s_k));
  int rc;
  x->tile_cap = 0;
  if((rc = x->d_tbytes.reset()) || (rc = x->d_tkept.reset()) || (rc = x->d_toff.reset())) return rc;
  const size_t cap = nb + nb / 8 + 16;
  if((rc = x->d_tbytes.alloc(cap)) || (rc = x->d_tkept.alloc(cap)) || (rc = x->d_toff.alloc(cap))) return rc;
  x->tile_cap = cap;
  return JFGPU_OK;
}

// The three launches for n > 0 positions, on s_k; the totals go to d_totals[2 * slot ..].  qtext_write_kernel writes nothing
// when the text is longer than cap_bytes.  The tile arrays hold (n + 255) / 256 entries (qtext_grow_tiles).
int qtext_launch(jfgpu_qtext* x, const uint8_t* d_bases, uint64_t n, const uint64_t* d_vals, const uint8_t* d_flags, uint8_t* d_text, uint64_t cap_bytes, int slot) {
  const uint32_t nb = (uint32_t)((n + kTextBlock - 1) / kTextBlock);
  const uint32_t lds = qtext_lds_in(x->job.k) + text_lds_out(x->job.line_max);
  const hipStream_t s_k = x->pipe.s_k;
  hipLaunchKernelGGL(qtext_len_kernel, dim3(nb), dim3(kTextBlock), 0, s_k, x->job, n, d_vals, d_flags, x->d_tbytes.get(), x->d_tkept.get());
  hipLaunchKernelGGL(text_scan_kernel, dim3(1), dim3(kTextBlock), 0, s_k, (const uint32_t*)x->d_tbytes, (const uint32_t*)x->d_tkept, nb, x->d_toff.get(),
                     x->d_totals + 2 * slot);
  return launch_lds(qtext_write_kernel, dim3(nb), dim3(kTextBlock), lds, s_k, x->job, d_bases, n, d_vals, d_flags, (const uint64_t*)x->d_toff,
                    (const uint64_t*)(x->d_totals + 2 * slot), cap_bytes, d_text);
}

constexpr uint64_t kQTextMaxPositions = (uint64_t)1 << 31;   // of one piece / one format_dev call: tiles are a 32-bit grid

// The host form over whoever answers: ask(d_bases, len, d_vals, d_flags) enqueues the look-up of a piece on `qs`.
template <class Ask>
int qtext_run(jfgpu_qtext* x, hipStream_t qs, const char* bases, size_t n, jfgpu_text_sink sink, void* user, Ask&& ask) {
  WindowPipe& P = x->pipe;
  int rc = P.begin_run(); if(rc) return rc;
  for(int i = 0; i < 4; ++i) x->counts[i] = 0;
  const uint32_t k = x->job.k, line_max = x->job.line_max;
  const uint64_t piece = x->piece_positions, step = piece - (k - 1);
  const uint64_t n_pieces = n == 0 ? 0 : n <= piece ? 1 : 1 + (n - piece + step - 1) / step;
  auto piece_len = [&](uint64_t i) { return std::min<uint64_t>(piece, n - i * step); };
  if(n_pieces) {
    // every buffer at the size of the largest piece, once: nothing grows while the pipeline runs
    const uint64_t pmax = piece_len(0);
    rc = qtext_grow_tiles(x, (size_t)((pmax + kTextBlock - 1) / kTextBlock)); if(rc) return rc;
    for(int s = 0; s < (n_pieces > 1 ? 2 : 1); ++s) {
      WindowPipe::Slot& S = P.slot[s];
      if((rc = S.d_raw.reserve((size_t)pmax + 64)) || (rc = S.d_out.reserve((size_t)pmax * line_max + 64)) || (rc = S.h_in.reserve((size_t)pmax)) ||
         (rc = x->d_vals[s].reserve((size_t)pmax)) || (rc = x->d_flags[s].reserve((size_t)pmax))) return rc;
    }
  }
  auto drain = [&](int code) { hipStreamSynchronize(qs); P.sync(); return code; };

  // the download and the sink of a piece whose kernels are enqueued
  auto finish = [&](uint64_t j) -> int {
    const int slot = (int)(j & 1);
    int frc = P.wait(slot); if(frc) return frc;
    const uint64_t nbytes = P.status_words(slot)[0], nlines = P.status_words(slot)[1];
    if(nlines > piece_len(j) || nbytes > nlines * line_max) return fail(JFGPU_E_HIP, "query text: the device wrote more than the piece can hold");
    x->counts[2] += nlines; x->counts[3] += nbytes;
    if(nbytes) {
      frc = P.download(slot, (size_t)nbytes); if(frc) return frc;
      if(P.sink([&] { return sink(user, (const char*)P.slot[slot].h_out.get(), nbytes, nlines); })) return fail(JFGPU_E_INVALID, "query text: the sink asked to stop");
    }
    return JFGPU_OK;
  };

  bool pending = false;
  for(uint64_t i = 0; i < n_pieces; ++i) {
    const int slot = (int)(i & 1);
    WindowPipe::Slot& S = P.slot[slot];
    const uint64_t len = piece_len(i);
    // ---- stage and upload (the kernels of piece i - 1 run meanwhile)
    const auto t0 = std::chrono::steady_clock::now();
    memcpy(S.h_in, bases + i * step, (size_t)len);
    rc = P.upload(slot, (size_t)len, t0); if(rc) return drain(rc);
    // ---- look-up on the answerer's stream, behind the upload; then the format kernels, behind the look-up.  The first k - 1
    // positions of a later piece are windows of the piece before: no line is made for a position below k - 1
    rc = P.kernels_begin(slot); if(rc) return drain(rc);
    { hipError_t e = hipStreamWaitEvent(qs, S.up_done, 0); if(e != hipSuccess) return drain(fail(JFGPU_E_HIP, hipGetErrorString(e))); }
    rc = ask((const char*)S.d_raw.get(), (size_t)len, x->d_vals[slot].get(), x->d_flags[slot].get()); if(rc) return drain(rc);
    {
      hipError_t e = hipEventRecord(x->asked[slot], qs);
      if(e == hipSuccess) e = hipStreamWaitEvent(P.s_k, x->asked[slot], 0);
      if(e != hipSuccess) return drain(fail(JFGPU_E_HIP, hipGetErrorString(e)));
    }
    rc = qtext_launch(x, S.d_raw, len, x->d_vals[slot], x->d_flags[slot], S.d_out, len * line_max, slot); if(rc) return drain(rc);
    if((rc = P.kernels_end(slot)) || (rc = P.status(slot, 0, x->d_totals + 2 * slot, 2 * sizeof(uint64_t))) || (rc = P.done(slot))) return drain(rc);
    x->counts[0] += 1; x->counts[1] += i ? len - (k - 1) : len;
    // ---- the piece before this one: download and sink while this one is looked up and formatted
    if(pending) { pending = false; rc = finish(i - 1); if(rc) return drain(rc); }
    pending = true;
  }
  if(pending) { rc = finish(n_pieces - 1); if(rc) return drain(rc); }
  return JFGPU_OK;
}

int qtext_args(const jfgpu_qtext* x, const char* bases, size_t n, jfgpu_text_sink sink, int device, uint32_t k, const char* who) {
  if(!sink) return fail(JFGPU_E_INVALID, "query text: no sink");
  if(n && !bases) return fail(JFGPU_E_INVALID, "query text: null buffer");
  if(x->device != device) return fail(JFGPU_E_INVALID, std::string("query text: the formatter lives on another device than the ") + who);
  if(x->job.k != k) return fail(JFGPU_E_INVALID, "query text: the formatter's k (" + std::to_string(x->job.k) + ") is not the " + who + "'s (" + std::to_string(k) + ")");
  return JFGPU_OK;
}

}  // namespace

extern "C" {

int jfgpu_qtext_create(const jfgpu_qtext_params* p, jfgpu_qtext** out) {
  if(!p || !out) return fail(JFGPU_E_INVALID, "null argument");
  *out = nullptr;
  if(p->k < 1 || p->k > 128) return fail(JFGPU_E_UNSUPPORTED, "query text: mer length must be in [1, 128]");
  const uint64_t env_piece = Tuning::from_env().query_piece;                    // (a switch below k means "as small as it goes")
  const uint64_t piece = p->piece_positions ? p->piece_positions : env_piece ? std::max<uint64_t>(env_piece, p->k) : kQueryTextPiecePositions;
  if(piece < p->k || piece > kQTextMaxPositions) return fail(JFGPU_E_INVALID, "query text: piece_positions must be in [k, 2^31]");
  int dev = 0;
  int rc = pick_device(p->device, &dev); if(rc) return rc;
  std::unique_ptr<jfgpu_qtext> x(new jfgpu_qtext);
  x->device = dev;
  x->job.k = p->k; x->job.line_max = p->k + 2 + 20;
  x->piece_positions = piece;
  if((rc = x->pipe.create(2 * sizeof(uint64_t))) || (rc = x->d_totals.alloc(4)) ||
     (rc = x->asked[0].create(hipEventDisableTiming)) || (rc = x->asked[1].create(hipEventDisableTiming))) return rc;
  *out = x.release();
  return JFGPU_OK;
}

void jfgpu_qtext_destroy(jfgpu_qtext* x) {
  if(!x) return;
  hipSetDevice(x->device);
  x->pipe.sync();
  delete x;
}

int jfgpu_qtext_line_max(const jfgpu_qtext* x, uint32_t* bytes) {
  if(!x || !bytes) return fail(JFGPU_E_INVALID, "null argument");
  *bytes = x->job.line_max;
  return JFGPU_OK;
}

int jfgpu_qtext_format_dev(jfgpu_qtext* x, const char* d_bases, size_t n, const uint64_t* d_vals, const uint8_t* d_flags,
                           char* d_text, uint64_t capacity_bytes, uint64_t* n_bytes, uint64_t* n_lines) {
  int rc = use_q(x); if(rc) return rc;
  if(!n_bytes || !n_lines) return fail(JFGPU_E_INVALID, "null argument");
  *n_bytes = *n_lines = 0;
  if(n == 0) return JFGPU_OK;
  if(!d_bases || !d_vals || !d_flags || (!d_text && capacity_bytes)) return fail(JFGPU_E_INVALID, "null argument");
  if((uintptr_t)d_vals & 7u) return fail(JFGPU_E_INVALID, "query text: the counts must start on an 8-byte boundary");
  if(n > kQTextMaxPositions) return fail(JFGPU_E_UNSUPPORTED, "query text: at most 2^31 positions a call");
  HIP_TRY(hipStreamSynchronize(x->pipe.s_k));
  rc = qtext_grow_tiles(x, (size_t)((n + kTextBlock - 1) / kTextBlock)); if(rc) return rc;
  rc = qtext_launch(x, (const uint8_t*)d_bases, n, d_vals, d_flags, (uint8_t*)d_text, capacity_bytes, 0); if(rc) return rc;
  HIP_TRY(hipGetLastError());
  uint64_t tot[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(tot, x->d_totals, sizeof tot, hipMemcpyDeviceToHost, x->pipe.s_k));
  HIP_TRY(hipStreamSynchronize(x->pipe.s_k));
  *n_bytes = tot[0]; *n_lines = tot[1];
  if(tot[0] > capacity_bytes)
    return fail(JFGPU_E_INVALID, "query text: the output needs " + std::to_string(tot[0]) + " bytes, the buffer holds " + std::to_string(capacity_bytes) + " (nothing was written)");
  return JFGPU_OK;
}

int jfgpu_query_text(jfgpu_table* t, jfgpu_qtext* x, const char* bases, size_t n, jfgpu_text_sink sink, void* user) {
  int rc = use(t); if(rc) return rc;
  if(!x) return fail(JFGPU_E_INVALID, "null query formatter");
  if(t->g.shard_bits) return fail(JFGPU_E_UNSUPPORTED, "query_text: not for a shard (the keys of the other shards are not here)");
  rc = qtext_args(x, bases, n, sink, t->device, t->g.k, "table"); if(rc) return rc;
  return qtext_run(x, t->stream, bases, n, sink, user,
                   [&](const char* d_bases, size_t len, uint64_t* d_vals, uint8_t* d_flags) { return jfgpu_query_ascii_dev(t, d_bases, len, d_vals, d_flags); });
}

int jfgpu_bc_query_text(jfgpu_bloom* b, jfgpu_qtext* x, const char* bases, size_t n, jfgpu_text_sink sink, void* user) {
  int rc = use_b(b); if(rc) return rc;
  if(!x) return fail(JFGPU_E_INVALID, "null query formatter");
  if(b->kind != 0) return fail(JFGPU_E_UNSUPPORTED, "query_text: a one-pass Bloom filter holds bits, not counts");
  rc = qtext_args(x, bases, n, sink, b->device, b->g.k, "Bloom counter"); if(rc) return rc;
  return qtext_run(x, b->stream, bases, n, sink, user,
                   [&](const char* d_bases, size_t len, uint64_t* d_vals, uint8_t* d_flags) { return jfgpu_bc_query_ascii_dev(b, d_bases, len, d_vals, d_flags); });
}

int jfgpu_qtext_last_ms(jfgpu_qtext* x, double out4[4]) {
  if(!x || !out4) return fail(JFGPU_E_INVALID, "null argument");
  for(int i = 0; i < 4; ++i) out4[i] = x->pipe.ms[i];
  return JFGPU_OK;
}

int jfgpu_qtext_counts(jfgpu_qtext* x, uint64_t out4[4]) {
  if(!x || !out4) return fail(JFGPU_E_INVALID, "null argument");
  for(int i = 0; i < 4; ++i) out4[i] = x->counts[i];
  return JFGPU_OK;
}

}  // extern "C"
