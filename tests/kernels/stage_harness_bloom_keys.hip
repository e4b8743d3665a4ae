// tests/kernels/stage_harness_bloom_keys.hip -- TEST INFRASTRUCTURE: the engine's translation unit plus one entry point
// (jfktb_p1) that launches P1b of the partitioned Bloom insert for keys of two, three and four words
// (p1_bloom_keys_kernel<WideTable | NTable, kBloomKeysPer>, kernels_bloom_part_keys.hip.hpp) ALONE, on a zeroed filter, with
// the caller's bucket bits, region size, grid and buffer bounds, and copies its outputs back.
//
// As tests/kernels/stage_harness.hip: the library built from this file is a superset of the engine, a counter made by ITS
// jfgpu_bc_create is what the launch takes and what read() reads back; never hand a handle made by one library to another.
// Nothing here is part of the product.  The template arguments and the dynamic-LDS size are the ones bloom_ingest launches.
//
// Two builds: hipcc --offload-arch=gfx950 (make kernel-harness-bloom-keys -> tests/kernels/_build/libjfgpu_ktbk.so) and
// g++ -DJFGPU_EMU -Itests/host/hip_emu (tests/host/build_ktbk_emu.sh -> tests/host/_build/libjfgpu_ktbk_emu.so).
#include "../../jellyfish_amd/csrc/jfgpu.hip"

namespace {

// device buffers of one call, freed when it returns
struct BKDevBufs {
  std::vector<void*> p;
  ~BKDevBufs() { for(void* q : p) hipFree(q); }
  template <typename T> int get(T** out, size_t n, int fill = -1) {
    *out = nullptr;
    void* q = nullptr;
    HIP_TRY(hipMalloc(&q, std::max<size_t>(n * sizeof(T), 16)));
    p.push_back(q);
    if(fill >= 0) HIP_TRY(hipMemset(q, fill, std::max<size_t>(n * sizeof(T), 16)));
    *out = (T*)q;
    return JFGPU_OK;
  }
  template <typename T> int put(T** out, const T* host, size_t n, size_t pad = 0) {
    int rc = get(out, n + pad, 0); if(rc) return rc;
    if(n) HIP_TRY(hipMemcpy(*out, host, n * sizeof(T), hipMemcpyHostToDevice));
    return JFGPU_OK;
  }
};
#define KTB_TRY(expr) do { int rc_ = (expr); if(rc_) return rc_; } while(0)

void bksay(char* dst, size_t len, const std::string& s) { if(dst && len) { strncpy(dst, s.c_str(), len - 1); dst[len - 1] = 0; } }

}  // namespace

extern "C" {

// 0 kPBlock  1 kGran  2 kPTilePos  3 kBloomSegBits  4 kBloomItemLow  5 kBloomKeysPer  6 kGranMaxB
uint64_t jfktb_const(int which) {
  switch(which) {
    case 0: return kPBlock;
    case 1: return kGran;
    case 2: return kPTilePos;
    case 3: return kBloomSegBits;
    case 4: return kBloomItemLow;
    case 5: return kBloomKeysPer;
    case 6: return kGranMaxB;
  }
  return 0;
}

// p1_bloom_keys_kernel over bases[lo, hi) (a contract buffer, its base 16-byte aligned) with 2^b1 buckets of 2^b2 segments,
// `grid` workgroups.  The counter: keys of two to four words, whole segments, mode 1, nothing pending.
// out: (2^b1 + 1) * cap items in and out (the last region is a guard); gcur: 2 * 2^b1 words out (cursors, overflow notes);
// tot: 2^b1; mers: what the launch added to the counter's k-mer count.
int jfktb_p1(jfgpu_bloom* b, uint32_t b1, uint32_t b2, uint32_t n_seg, const uint8_t* bases, uint64_t n_bases, int64_t lo, int64_t hi,
             uint32_t cap, uint32_t grid, uint32_t* out, uint32_t* gcur, uint64_t* tot, uint64_t* mers, char* launched, size_t launched_len) {
  int rc = use_b(b); if(rc) return rc;
  if(b->kind != 0 || !b->part_ok || b->mode != 1 || !b->pending.empty() || !(b->wide || b->nword))
    return fail(JFGPU_E_INVALID, "jfktb_p1: a Bloom counter of two- to four-word keys with whole segments, in mode 1, nothing pending");
  if(n_seg != b->bp.n_seg || b1 > 10 || b2 > 11 || ((uint64_t)1 << (b1 + b2)) < n_seg)
    return fail(JFGPU_E_INVALID, "jfktb_p1: n_seg is the filter's own, b1 <= 10, b2 <= 11, n_seg <= 2^(b1 + b2)");
  if(!grid || grid > 64) return fail(JFGPU_E_INVALID, "jfktb_p1: 1 <= grid <= 64");
  if(lo < 0 || hi < lo || (uint64_t)hi > n_bases) return fail(JFGPU_E_INVALID, "jfktb_p1: [lo, hi) outside the buffer");
  if(cap % kGran || !cap) return fail(JFGPU_E_INVALID, "jfktb_p1: regions are whole reservations");
  const BloomPart BP{b1, b2, n_seg, 0};
  const uint32_t nb = 1u << b1;
  BKDevBufs D;
  uint8_t* d_bases; uint32_t* d_out; unsigned int* d_gcur; unsigned long long* d_tot;
  KTB_TRY(D.put(&d_bases, bases, (size_t)n_bases, 32));
  KTB_TRY(D.put(&d_out, out, ((size_t)nb + 1) * cap));
  KTB_TRY(D.get(&d_gcur, 2 * (size_t)nb, 0));
  KTB_TRY(D.get(&d_tot, nb, 0));
  unsigned long long m0 = 0, m1 = 0;
  HIP_TRY(hipMemcpy(&m0, b->d_mers, 8, hipMemcpyDeviceToHost));
  const DevBloom B = b->view();
  const size_t lds = p1_bloom_keys_lds(b->g.nbytes);                                    // (bloom_ingest)
  if(b->nword) KTB_TRY(launch_lds(p1_bloom_keys_kernel<NTable, kBloomKeysPer>, dim3(grid), dim3(kPBlock), lds, b->stream, B, BP, b->ng, (const uint8_t*)d_bases, lo, hi, cap,
                                  d_gcur, d_tot, d_out, b->d_mers));
  else         KTB_TRY(launch_lds(p1_bloom_keys_kernel<WideTable, kBloomKeysPer>, dim3(grid), dim3(kPBlock), lds, b->stream, B, BP, b->wg, (const uint8_t*)d_bases, lo, hi, cap,
                                  d_gcur, d_tot, d_out, b->d_mers));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(b->stream));
  HIP_TRY(hipMemcpy(&m1, b->d_mers, 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out, d_out, ((size_t)nb + 1) * cap * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(gcur, d_gcur, 2 * (size_t)nb * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(tot, d_tot, (size_t)nb * 8, hipMemcpyDeviceToHost));
  if(mers) *mers = m1 - m0;
  bksay(launched, launched_len, std::string("p1_bloom_keys_kernel<") + (b->nword ? "NTable" : "WideTable") + "," + std::to_string(kBloomKeysPer) + ">");
  return JFGPU_OK;
}

}  // extern "C"
