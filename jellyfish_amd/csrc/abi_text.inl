// jellyfish_amd/csrc/abi_text.inl -- C ABI of the device text formatter (jfgpu_text_*, jfgpu_dump_next_text), included by
// jfgpu.hip.  Kernels: kernels_text.hip.hpp.  The host side here owns the windows of jfgpu_text_run (fixed numbers of
// records, records have one width); the two-deep pipeline of uploads, kernels and downloads is a WindowPipe (hip_own.hpp),
// the one under abi_merge.inl.
struct jfgpu_text {
  int device = 0;
  WindowPipe pipe;                                          // (first: its streams outlive the buffers below)
  TextJob job{};
  uint64_t window_records = 0;
  DevBuf<uint32_t> d_tbytes, d_tkept; DevBuf<uint64_t> d_toff; size_t tile_cap = 0;
  DevBuf<uint64_t> d_totals;                                // [2][2]: bytes and lines of the window in each slot (a slot's status block)
  uint64_t counts[4] = {0, 0, 0, 0};                        // windows, records read, records kept, bytes written
};

namespace {

int use_x(const jfgpu_text* x) { return use_dev(x, "null text formatter"); }

int text_grow_tiles(jfgpu_text* x, size_t nb) {
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

// The three launches for n > 0 records at d_rec, on s_k; the totals go to d_totals[2 * slot ..].  text_write_kernel writes
// nothing when the text is longer than cap_bytes.  The tile arrays hold (n + 255) / 256 entries (text_grow_tiles).
int text_launch(jfgpu_text* x, const uint8_t* d_rec, uint64_t n, uint8_t* d_text, uint64_t cap_bytes, int slot) {
  const uint32_t nb = (uint32_t)((n + kTextBlock - 1) / kTextBlock);
  const uint32_t lds_raw = text_lds_raw(x->job.rb), lds_out = text_lds_out(x->job.line_max);
  const hipStream_t s_k = x->pipe.s_k;
  int rc = launch_lds(text_len_kernel, dim3(nb), dim3(kTextBlock), lds_raw, s_k, x->job, d_rec, n, x->d_tbytes.get(), x->d_tkept.get());
  if(rc) return rc;
  hipLaunchKernelGGL(text_scan_kernel, dim3(1), dim3(kTextBlock), 0, s_k, (const uint32_t*)x->d_tbytes, (const uint32_t*)x->d_tkept, nb, x->d_toff.get(),
                     x->d_totals + 2 * slot);
  return launch_lds(text_write_kernel, dim3(nb), dim3(kTextBlock), lds_raw + lds_out, s_k, x->job, d_rec, n, (const uint64_t*)x->d_toff,
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
  int dev = 0;
  int rc = pick_device(p->device, &dev); if(rc) return rc;
  std::unique_ptr<jfgpu_text> x(new jfgpu_text);
  x->device = dev;
  TextJob& J = x->job;
  J.k = p->k; J.kb = (2 * p->k + 7) / 8; J.vb = p->counter_len; J.rb = J.kb + J.vb;
  J.layout = p->layout; J.sep = p->layout == JFGPU_TEXT_COLUMN ? p->separator : (uint32_t)' '; J.pad_ = 0;
  J.lower = p->lower; J.upper = p->upper;
  const uint64_t vmax = J.vb >= 8 ? ~0ull : ((1ull << (8 * J.vb)) - 1);
  J.line_max = J.k + 2 + text_digits(std::min(vmax, p->upper)) + (J.layout == kTextFasta ? 1 : 0);
  x->window_records = p->window_records ? p->window_records : kTextWindowRecords;
  if((rc = x->pipe.create(2 * sizeof(uint64_t))) || (rc = x->d_totals.alloc(4))) return rc;
  *out = x.release();
  return JFGPU_OK;
}

void jfgpu_text_destroy(jfgpu_text* x) {
  if(!x) return;
  hipSetDevice(x->device);
  x->pipe.sync();
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
  WindowPipe& P = x->pipe;
  rc = P.begin_run(); if(rc) return rc;
  for(int i = 0; i < 4; ++i) x->counts[i] = 0;
  const uint32_t rb = x->job.rb, line_max = x->job.line_max;
  const uint64_t W = x->window_records;
  const uint64_t n_win = (n_records + W - 1) / W;
  auto win_n = [&](uint64_t i) { return std::min<uint64_t>(W, n_records - i * W); };
  if(n_win) {
    // every buffer at the size of the largest window, once: nothing grows while the pipeline runs
    const uint64_t wmax = win_n(0);
    rc = text_grow_tiles(x, (size_t)((wmax + kTextBlock - 1) / kTextBlock)); if(rc) return rc;
    for(int s = 0; s < (n_win > 1 ? 2 : 1); ++s) {
      WindowPipe::Slot& S = P.slot[s];
      if((rc = S.d_raw.reserve((size_t)wmax * rb + 64)) ||               // (read to the next 16-byte boundary)
         (rc = S.d_out.reserve((size_t)wmax * line_max + 64)) || (rc = S.h_in.reserve((size_t)wmax * rb))) return rc;
    }
  }

  // the download and the sink of a window whose kernels are enqueued
  auto finish = [&](uint64_t j) -> int {
    const int slot = (int)(j & 1);
    int frc = P.wait(slot); if(frc) return frc;
    const uint64_t nbytes = P.status_words(slot)[0], nkept = P.status_words(slot)[1];
    if(nkept > win_n(j) || nbytes > nkept * line_max) return fail(JFGPU_E_HIP, "text: the device wrote more than the window can hold");
    x->counts[2] += nkept; x->counts[3] += nbytes;
    if(nbytes) {
      frc = P.download(slot, (size_t)nbytes); if(frc) return frc;
      if(P.sink([&] { return sink(user, (const char*)P.slot[slot].h_out.get(), nbytes, nkept); })) return fail(JFGPU_E_INVALID, "text: the sink asked to stop");
    }
    return JFGPU_OK;
  };

  bool pending = false;
  for(uint64_t i = 0; i < n_win; ++i) {
    const int slot = (int)(i & 1);
    WindowPipe::Slot& S = P.slot[slot];
    const uint64_t n = win_n(i);
    // ---- stage and upload (the kernels of window i - 1 run meanwhile)
    const auto t0 = std::chrono::steady_clock::now();
    memcpy(S.h_in, (const uint8_t*)body + i * W * rb, (size_t)n * rb);
    rc = P.upload(slot, (size_t)n * rb, t0); if(rc) return rc;
    // ---- kernels
    rc = P.kernels_begin(slot); if(rc) return rc;
    rc = text_launch(x, S.d_raw, n, S.d_out, n * line_max, slot); if(rc) return rc;
    if((rc = P.kernels_end(slot)) || (rc = P.status(slot, 0, x->d_totals + 2 * slot, 2 * sizeof(uint64_t))) || (rc = P.done(slot))) return rc;
    x->counts[0] += 1; x->counts[1] += n;
    // ---- the window before this one: download and sink while this one's kernels run
    if(pending) { pending = false; rc = finish(i - 1); if(rc) { hipStreamSynchronize(P.s_k); return rc; } }
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
  HIP_TRY(hipStreamSynchronize(x->pipe.s_k));
  rc = text_grow_tiles(x, (size_t)((n_records + kTextBlock - 1) / kTextBlock)); if(rc) return rc;
  rc = text_launch(x, (const uint8_t*)d_records, n_records, (uint8_t*)d_text, capacity_bytes, 0); if(rc) return rc;
  HIP_TRY(hipGetLastError());
  uint64_t tot[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(tot, x->d_totals, sizeof tot, hipMemcpyDeviceToHost, x->pipe.s_k));
  HIP_TRY(hipStreamSynchronize(x->pipe.s_k));
  *n_bytes = tot[0]; *n_kept = tot[1];
  if(tot[0] > capacity_bytes)
    return fail(JFGPU_E_INVALID, "text: the output needs " + std::to_string(tot[0]) + " bytes, the buffer holds " + std::to_string(capacity_bytes) + " (nothing was written)");
  return JFGPU_OK;
}

int jfgpu_text_last_ms(jfgpu_text* x, double out4[4]) {
  if(!x || !out4) return fail(JFGPU_E_INVALID, "null argument");
  for(int i = 0; i < 4; ++i) out4[i] = x->pipe.ms[i];
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
  HIP_TRY(hipStreamSynchronize(x->pipe.s_k));
  const uint64_t cursor = t->dump_tile_cursor;
  uint64_t nrec = 0;
  rc = dump_next_chunk(t, cap_rec, &nrec); if(rc) return rc;
  if(!nrec) return JFGPU_OK;
  // a failure from here on leaves the chunk undelivered: the cursor goes back, the next call produces it again
  auto undo = [&](int code) { t->dump_tile_cursor = cursor; hipStreamSynchronize(t->stream); return code; };
  if((rc = text_grow_tiles(x, (size_t)((nrec + kTextBlock - 1) / kTextBlock))) || (rc = x->pipe.slot[0].d_out.reserve((size_t)nrec * x->job.line_max + 64)))
    return undo(rc);
  hipError_t e = hipStreamSynchronize(t->stream);                  // the chunk is in d_dump
  uint64_t tot[2] = {0, 0};
  if(e == hipSuccess) {
    rc = text_launch(x, t->d_dump, nrec, x->pipe.slot[0].d_out, nrec * x->job.line_max, 0); if(rc) return undo(rc);
    e = hipGetLastError();
  }
  if(e == hipSuccess) e = hipMemcpyAsync(tot, x->d_totals, sizeof tot, hipMemcpyDeviceToHost, x->pipe.s_k);
  if(e == hipSuccess) e = hipStreamSynchronize(x->pipe.s_k);
  if(e == hipSuccess && (tot[1] > nrec || tot[0] > capacity_bytes))
    return undo(fail(JFGPU_E_HIP, "dump_next_text: the device wrote more than the chunk can hold"));
  if(e == hipSuccess && tot[0]) e = hipMemcpyAsync(out, x->pipe.slot[0].d_out, tot[0], hipMemcpyDeviceToHost, x->pipe.s_k);
  if(e == hipSuccess) e = hipStreamSynchronize(x->pipe.s_k);
  if(e != hipSuccess) return undo(fail(JFGPU_E_HIP, hipGetErrorString(e)));
  *n_records = nrec; *n_bytes = tot[0];
  return JFGPU_OK;
}

}  // extern "C"
