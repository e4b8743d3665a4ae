// tests/kernels/stage_harness_nword.hip -- TEST INFRASTRUCTURE: the engine's translation unit plus entry points (jfktn_*)
// that launch ONE stage of the partitioned insert of three- and four-word keys (kernels_nword_part.hip.hpp) with the
// caller's arguments and copy its outputs back: P1n (p1_nword_granule_kernel), the exact P2 on 256-bit items (p2_kernel +
// scan_matrix_kernel + p2_scatter_sorted_kernel with ITEM = u256) and Tn (tile_insert_nword_kernel, items_direct_nword_kernel).
//
// As tests/kernels/stage_harness.hip: the library built from this file is a superset of the engine, a table made by ITS
// jfgpu_create is what the launches take and what look-up / stats / digest read back; never hand a handle made by one
// library to another.  Nothing here is part of the product.  Template arguments are the ones host_partition.inl launches.
// Items are four 64-bit words, lowest first.
//
// Two builds: hipcc --offload-arch=gfx950 (make kernel-harness-nword -> tests/kernels/_build/libjfgpu_ktn.so) and
// g++ -DJFGPU_EMU -Itests/host/hip_emu (tests/host/build_ktn_emu.sh -> tests/host/_build/libjfgpu_ktn_emu.so).
#include "../../jellyfish_amd/csrc/jfgpu.hip"

namespace {

// device buffers of one call, freed when it returns
struct NDevBufs {
  std::vector<void*> p;
  ~NDevBufs() { for(void* q : p) hipFree(q); }
  template <typename T> int get(T** out, size_t n, int fill = -1) {
    *out = nullptr;
    void* q = nullptr;
    HIP_TRY(hipMalloc(&q, std::max<size_t>(n * sizeof(T), 32)));
    p.push_back(q);
    if(fill >= 0) HIP_TRY(hipMemset(q, fill, std::max<size_t>(n * sizeof(T), 32)));
    *out = (T*)q;
    return JFGPU_OK;
  }
  template <typename T> int put(T** out, const T* host, size_t n, size_t pad = 0) {
    int rc = get(out, n + pad, 0); if(rc) return rc;
    if(n) HIP_TRY(hipMemcpy(*out, host, n * sizeof(T), hipMemcpyHostToDevice));
    return JFGPU_OK;
  }
};
#define KTN_TRY(expr) do { int rc_ = (expr); if(rc_) return rc_; } while(0)

void nsay(char* dst, size_t len, const std::string& s) { if(dst && len) { strncpy(dst, s.c_str(), len - 1); dst[len - 1] = 0; } }

int ktn_table(jfgpu_table* t, const char* who) {
  int rc = use(t); if(rc) return rc;
  if(!t->nword || !t->item256 || t->nt.bloom.data || t->g.shard_bits) return fail(JFGPU_E_INVALID, std::string(who) + ": keys of three and four words with the partitioned geometry, no filter, no shard");
  return JFGPU_OK;
}

// the segments of a launch on the device; every unit's range is checked against its segment first
int ktn_segments(NDevBufs& D, SegList& S, const char* who, uint32_t n_seg, const void* const* seg_items, const uint64_t* n_items, const uint64_t* const* seg_off,
                 const uint64_t* n_off, const uint32_t* sh, uint32_t unit0, uint32_t n_units) {
  if(!n_seg || n_seg > 3 || !n_units) return fail(JFGPU_E_INVALID, std::string(who) + ": one to three segments, at least one unit");
  memset(&S, 0, sizeof S);
  S.n = n_seg;
  for(uint32_t s = 0; s < n_seg; ++s) {
    if(sh[s] > 1 || n_off[s] < (((uint64_t)unit0 + n_units - 1) << sh[s]) + 2) return fail(JFGPU_E_INVALID, std::string(who) + ": offsets do not cover the units");
    for(uint32_t u = unit0; u < unit0 + n_units; ++u) {
      const uint64_t a = seg_off[s][(size_t)u << sh[s]], b = seg_off[s][((size_t)u << sh[s]) + 1];
      if(a > b || b > n_items[s]) return fail(JFGPU_E_INVALID, std::string(who) + ": a unit's range lies outside the items");
    }
    uint64_t *di, *doff;
    KTN_TRY(D.put(&di, (const uint64_t*)seg_items[s], (size_t)n_items[s] * 4, 4));
    KTN_TRY(D.put(&doff, seg_off[s], (size_t)n_off[s]));
    S.items[s] = di; S.off[s] = doff; S.sh[s] = sh[s];
  }
  return JFGPU_OK;
}

}  // namespace

extern "C" {

// 0 kPBlock  1 kGran  2 kNChunk  3 kNTileBlock  4 kP2NWordPer  5 kNTileBits  6 kPTilePos  7 kNLoBits  8 sizeof(u256)
uint64_t jfktn_const(int which) {
  switch(which) {
    case 0: return kPBlock;
    case 1: return kGran;
    case 2: return kNChunk;
    case 3: return kNTileBlock;
    case 4: return kP2NWordPer;
    case 5: return kNTileBits;
    case 6: return kPTilePos;
    case 7: return kNLoBits;
    case 8: return sizeof(u256);
  }
  return 0;
}

// 0 lsize_l 1 tile_bits 2 rem_bits 3 tag_bits 4 cnt_bits 5 nbytes 6 returning 7 part_ok 8 b1 9 b2 10 rest_shift 11 item_bits
// 12 lsize_g 13 canonical 14 tag_full 15 key_bits 16 max_probe 17 item256
int jfktn_geom(jfgpu_table* t, uint64_t* out, uint32_t n) {
  if(!t || !out) return fail(JFGPU_E_INVALID, "null argument");
  const uint64_t v[18] = {t->g.lsize_l, t->g.tile_bits, t->g.rem_bits, t->g.tag_bits, t->g.cnt_bits, t->g.nbytes, (uint64_t)t->returning, (uint64_t)t->part_ok,
                          t->pg.b1, t->pg.b2, t->pg.rest_shift, t->pg.item_bits, t->g.lsize_g, t->g.canonical, t->nt.N.tag_full, t->g.key_bits, t->nt.max_probe,
                          (uint64_t)t->item256};
  for(uint32_t i = 0; i < n && i < 18; ++i) out[i] = v[i];
  return JFGPU_OK;
}

// ---- P1n alone --------------------------------------------------------------------------------------------------------
// p1_nword_granule_kernel<table's RETURNING> over bases[lo, hi) with 2^b1 buckets, `grid` workgroups; b2 = what is left of
// the tile index.  What a region cannot take is claimed in the table itself (nword_item_direct), which needs the buckets
// to be groups of whole tiles: b1 <= the table's tile-index bits.
// out: (2^b1 + 1) * cap items of four words in and out (the last region is a guard); gcur: 2 * 2^b1 words out; tot: 2^b1 out;
// ctr[2]: what the kernel added to the table's k-mer counter and to its direct counter.
int jfktn_p1(jfgpu_table* t, uint32_t b1, const uint8_t* bases, uint64_t n_bases, int64_t lo, int64_t hi, uint32_t cap, uint32_t grid,
             uint64_t* out, uint32_t* gcur, uint64_t* tot, uint64_t* ctr, char* launched, size_t launched_len) {
  KTN_TRY(ktn_table(t, "jfktn_p1"));
  const uint32_t tbits = t->g.lsize_l - t->g.tile_bits;
  if(b1 > 10 || b1 > tbits || !grid || grid > 64) return fail(JFGPU_E_INVALID, "jfktn_p1: 0 <= b1 <= min(10, tile-index bits), 1 <= grid <= 64");
  if(lo < 0 || hi < lo || (uint64_t)hi > n_bases) return fail(JFGPU_E_INVALID, "jfktn_p1: [lo, hi) outside the buffer");
  if(cap % kGran || !cap) return fail(JFGPU_E_INVALID, "jfktn_p1: regions are whole reservations");
  PartGeom P;
  P.b1 = b1; P.b2 = tbits - b1;
  P.rest_shift = t->g.lsize_l - b1; P.item_bits = P.rest_shift + t->g.rem_bits;
  if(P.item_bits >= 256) return fail(JFGPU_E_INVALID, "jfktn_p1: the geometry's items do not fit 255 bits");
  const uint32_t nb = 1u << b1;
  NDevBufs D;
  uint8_t* d_bases; uint64_t* d_out; unsigned int* d_gcur; unsigned long long* d_tot;
  KTN_TRY(D.put(&d_bases, bases, (size_t)n_bases, 32));
  KTN_TRY(D.put(&d_out, out, ((size_t)nb + 1) * cap * 4));
  KTN_TRY(D.get(&d_gcur, 2 * (size_t)nb, 0));
  KTN_TRY(D.get(&d_tot, nb, 0));
  uint64_t c0[CTR_COUNT], c1[CTR_COUNT];
  KTN_TRY(read_counters(t, c0));
  const size_t lds = p1_nword_lds(t->g.nbytes);                                      // (p1_plan)
  if(t->returning) KTN_TRY(launch_lds(p1_nword_granule_kernel<true>, dim3(grid), dim3(kPBlock), lds, t->stream, t->nt, P, (const uint8_t*)d_bases, lo, hi, cap, d_gcur, d_tot, (u256*)d_out));
  else             KTN_TRY(launch_lds(p1_nword_granule_kernel<false>, dim3(grid), dim3(kPBlock), lds, t->stream, t->nt, P, (const uint8_t*)d_bases, lo, hi, cap, d_gcur, d_tot, (u256*)d_out));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(t->stream));
  t->pristine = false;
  KTN_TRY(read_counters(t, c1));
  HIP_TRY(hipMemcpy(out, d_out, ((size_t)nb + 1) * cap * 32, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(gcur, d_gcur, 2 * (size_t)nb * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(tot, d_tot, (size_t)nb * 8, hipMemcpyDeviceToHost));
  if(ctr) { ctr[0] = c1[CTR_MERS] - c0[CTR_MERS]; ctr[1] = c1[CTR_DIRECT] - c0[CTR_DIRECT]; }
  nsay(launched, launched_len, std::string("p1_nword_granule_kernel<") + (t->returning ? "true" : "false") + ">");
  return JFGPU_OK;
}

// ---- the exact P2 on 256-bit items alone --------------------------------------------------------------------------------
// p2_kernel<u256, false>, scan_matrix_kernel, p2_scatter_sorted_kernel<u256, kP2NWordPer>, 32 workgroups a bucket, over P1
// buckets [bucket0, bucket0 + nbk); base[q]: where bucket q's items start in out.  Segments: unit j of segment s is
// items[off[j << sh] .. off[(j << sh) + 1]); sh = 1: a granule batch, all-ones items are holes.
// out: n_out items in and out; goff: n_dest + 1 words in and out.
int jfktn_p2(jfgpu_table* t, uint32_t b2e, uint32_t tag_bits, uint32_t n_seg, const void* const* seg_items, const uint64_t* n_items,
             const uint64_t* const* seg_off, const uint64_t* n_off, const uint32_t* sh, uint32_t bucket0, uint32_t nbk, uint32_t n_dest,
             const uint64_t* base, uint64_t* out, uint64_t n_out, uint64_t* goff, char* launched, size_t launched_len) {
  KTN_TRY(ktn_table(t, "jfktn_p2"));
  if(b2e > 11 || tag_bits + b2e > 256 || !base) return fail(JFGPU_E_INVALID, "jfktn_p2: at most 2048 destinations a bucket, inside the item; base is needed");
  if(((uint64_t)(bucket0 + nbk) << b2e) > n_dest) return fail(JFGPU_E_INVALID, "jfktn_p2: launched destinations beyond n_dest");
  NDevBufs D;
  SegList S;
  KTN_TRY(ktn_segments(D, S, "jfktn_p2", n_seg, seg_items, n_items, seg_off, n_off, sh, bucket0, nbk));
  for(uint32_t j = bucket0; j < bucket0 + nbk; ++j) {      // every launched bucket's items inside out
    uint64_t n = 0;
    for(uint32_t s = 0; s < n_seg; ++s) n += seg_off[s][((size_t)j << sh[s]) + 1] - seg_off[s][(size_t)j << sh[s]];
    if(n >> 32 || base[j] + n > n_out) return fail(JFGPU_E_INVALID, "jfktn_p2: a bucket's items do not fit out behind base");
  }
  const int g2 = 32;
  const uint32_t nb1 = bucket0 + nbk, nb2e = 1u << b2e;
  uint64_t *d_out, *d_goff, *d_base; uint32_t* d_M2;
  KTN_TRY(D.put(&d_out, out, (size_t)n_out * 4));
  KTN_TRY(D.get(&d_M2, (size_t)nb1 * g2 * nb2e, 0));
  KTN_TRY(D.put(&d_goff, goff, (size_t)n_dest + 1));
  KTN_TRY(D.put(&d_base, base, nb1));
  PartGeom pg2; memset(&pg2, 0, sizeof pg2);
  pg2.b2 = b2e;
  const dim3 grid(g2, nbk), block(kPBlock);
  hipLaunchKernelGGL((p2_kernel<u256, false>), grid, block, 0, t->stream, pg2, tag_bits, S, d_M2, (const uint64_t*)d_goff, (u256*)d_out, bucket0);
  hipLaunchKernelGGL(scan_matrix_kernel, dim3(nbk), dim3(1024), 0, t->stream, d_M2, (uint32_t)g2, nb2e, (const uint64_t*)d_base, d_goff, bucket0);
  KTN_TRY(launch_lds(p2_scatter_sorted_kernel<u256, kP2NWordPer>, grid, block, (size_t)kPBlock * kP2NWordPer * sizeof(u256), t->stream, pg2, tag_bits, S,
                     (const uint32_t*)d_M2, (const uint64_t*)d_goff, (u256*)d_out, bucket0));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(t->stream));
  HIP_TRY(hipMemcpy(goff, d_goff, ((size_t)n_dest + 1) * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out, d_out, (size_t)n_out * 32, hipMemcpyDeviceToHost));
  nsay(launched, launched_len, "p2_kernel<u256,false>+scan_matrix_kernel+p2_scatter_sorted_kernel<u256,kP2NWordPer>");
  return JFGPU_OK;
}

// ---- Tn alone ---------------------------------------------------------------------------------------------------------
// kernel 0: tile_insert_nword_kernel<table's RETURNING> over n_units tiles from tile0, 1 to 3 segments whose unit u is tile
//           tile0 + u;  kernel 1: items_direct_nword_kernel<table's RETURNING> over one granule batch of the table's own P1
//           geometry (segment 0: 2^b1 regions of `cap` items and their (begin, end) pairs).
// ctr[2]: what the launch added to the table's tile-full counter and to its side-table entries.
int jfktn_tile(jfgpu_table* t, int kernel, uint32_t n_seg, const void* const* seg_items, const uint64_t* n_items, const uint64_t* const* seg_off,
               const uint64_t* n_off, const uint32_t* sh, uint64_t tile0, uint32_t n_units, uint32_t grid, uint64_t cap, uint64_t* ctr,
               char* launched, size_t launched_len) {
  KTN_TRY(ktn_table(t, "jfktn_tile"));
  if(kernel < 0 || kernel > 1 || !grid) return fail(JFGPU_E_INVALID, "jfktn_tile: bad kernel or grid");
  const uint64_t nb = 1ull << t->pg.b1;
  if(kernel == 1) {
    if(n_seg != 1 || !cap || sh[0] != 1 || n_items[0] != nb * cap || n_off[0] < 2 * nb) return fail(JFGPU_E_INVALID, "jfktn_tile: a granule batch is 2^b1 regions of cap items");
    for(uint64_t b = 0; b < nb; ++b) if(seg_off[0][2 * b + 1] > (b + 1) * cap) return fail(JFGPU_E_INVALID, "jfktn_tile: a region ends beyond itself");
  } else if(!n_units || tile0 + n_units > n_tiles_of(t)) return fail(JFGPU_E_INVALID, "jfktn_tile: units beyond the table");
  NDevBufs D;
  SegList S;
  KTN_TRY(ktn_segments(D, S, "jfktn_tile", n_seg, seg_items, n_items, seg_off, n_off, sh, 0, kernel == 1 ? (uint32_t)nb : n_units));
  uint64_t c0[CTR_COUNT], c1[CTR_COUNT];
  KTN_TRY(read_counters(t, c0));
  const bool rt = t->returning;
  std::string name;
  if(kernel == 0) {
    const dim3 g(std::min(grid, n_units)), block(kNTileBlock);
    const size_t tile_lds = (size_t)32 << t->g.tile_bits;                             // (launch_tile_kernel)
    if(rt) KTN_TRY(launch_lds(tile_insert_nword_kernel<true>, g, block, tile_lds, t->stream, t->nt, S, tile0, n_units));
    else   KTN_TRY(launch_lds(tile_insert_nword_kernel<false>, g, block, tile_lds, t->stream, t->nt, S, tile0, n_units));
    name = std::string("tile_insert_nword_kernel<") + (rt ? "true" : "false") + ">";
  } else {
    const dim3 g(grid), block(kBlock);
    if(rt) hipLaunchKernelGGL(items_direct_nword_kernel<true>, g, block, 0, t->stream, t->nt, t->pg, (const u256*)S.items[0], S.off[0], cap);
    else   hipLaunchKernelGGL(items_direct_nword_kernel<false>, g, block, 0, t->stream, t->nt, t->pg, (const u256*)S.items[0], S.off[0], cap);
    name = std::string("items_direct_nword_kernel<") + (rt ? "true" : "false") + ">";
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(t->stream));
  t->pristine = false;
  KTN_TRY(read_counters(t, c1));
  if(ctr) { ctr[0] = c1[CTR_FULL] - c0[CTR_FULL]; ctr[1] = c1[CTR_OVF_USED] - c0[CTR_OVF_USED]; }
  // (a full tile is this launch's finding, not the table's: the next jfgpu_sync must not report "Hash full")
  if(c1[CTR_FULL] != c0[CTR_FULL]) HIP_TRY(hipMemcpy(&t->dt.counters[CTR_FULL], &c0[CTR_FULL], 8, hipMemcpyHostToDevice));
  nsay(launched, launched_len, name);
  return JFGPU_OK;
}

}  // extern "C"
