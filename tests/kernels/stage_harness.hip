// tests/kernels/stage_harness.hip -- TEST INFRASTRUCTURE: the engine's translation unit plus entry points (jfkt_*) that
// launch ONE stage of the partitioned insert path -- P1 (p1_ring_kernel), P2 (p2_ring_roles_kernel / p2_ring_kernel, each
// followed by p1_stragglers_kernel), T (tile_rank_insert_kernel) -- with the caller's arguments and copy its outputs back.
// Likewise the sort-based P2 at 4-, 8- and 16-byte items (jfkt_p2_sort: p2_granule_kernel + granule_finish[_range]_kernel;
// p2_kernel + scan_matrix_kernel + p2_scatter_sorted_kernel) and the two-word path's own stages (jfkt_p1_wide:
// p1_wide_granule_kernel; jfkt_tile_wide: tile_insert_wide_kernel, tile_insert_wide_pipe_kernel, items_direct_wide_kernel).
// And the partitioned Bloom insert (jfkt_bloom_p1: the three P1b families; jfkt_bloom_seg: bloom_segment_kernel;
// jfkt_bloom_items_direct; jfkt_bloom_p2: the P2 kernels with the Bloom functors), on a Bloom counter of this library.
//
// The engine is one translation unit, so including it here gives the harness the anonymous namespace, jfgpu_table, the
// descriptors and the kernels.  The library built from this file is a superset of the engine: a table made by ITS
// jfgpu_create is what the launches take and what lookup / dump / stats / digest read back.  Never hand a handle made by
// one library to the other.  Nothing here is part of the product; the product library does not change.
//
// The ring kernels are instantiated with a DIRECT functor that RECORDS its calls -- (destination, item, occurrences) into
// a list with a counter -- so that what the product inserts with global atomics (a side effect somewhere in a table)
// becomes an output a test can compare.  Template arguments are the ones host_partition.inl launches.
//
// Two builds: hipcc --offload-arch=gfx950 (make kernel-harness -> tests/kernels/_build/libjfgpu_kt.so) and
// g++ -DJFGPU_EMU -Itests/host/hip_emu (tests/host/build_kt_emu.sh -> tests/host/_build/libjfgpu_kt_emu.so).
#include "../../jellyfish_amd/csrc/jfgpu.hip"

namespace {

// DIRECT of the ring kernels and of p1_stragglers_kernel: the call is written down, nothing is inserted
struct RecordDirect {
  static constexpr bool kCountsDirect = true;
  uint64_t* rec; unsigned long long* n; uint64_t cap;          // rec[3 i]: destination, item, occurrences
  __device__ void operator()(uint32_t dest, uint64_t item, uint32_t cnt) const {
    const unsigned long long at = atomicAdd(n, 1ull);
    if(at < cap) { rec[3 * at] = dest; rec[3 * at + 1] = item; rec[3 * at + 2] = cnt; }
  }
};

// DIRECT of p2_granule_kernel (called with the P1 bucket and the item): destination, low word, high word; the kernel adds
// its count of such calls to direct_counter(), which is the harness's own
template <typename ITEM>
struct RecordDirectT {
  uint64_t* rec; unsigned long long* n; uint64_t cap; unsigned long long* ctr; uint32_t b2e, tag_bits;
  __device__ void operator()(uint32_t bucket, ITEM item) const {
    const unsigned long long at = atomicAdd(n, 1ull);
    if(at < cap) {
      rec[3 * at] = ((uint64_t)bucket << b2e) | ((uint64_t)(item >> tag_bits) & ((1ull << b2e) - 1));
      rec[3 * at + 1] = (uint64_t)item;
      if constexpr(sizeof(ITEM) == 16) rec[3 * at + 2] = (uint64_t)(item >> 64); else rec[3 * at + 2] = 0;
    }
  }
  __device__ unsigned long long* direct_counter() const { return ctr; }
};

// device buffers of one call, freed when it returns
struct DevBufs {
  std::vector<void*> p;
  ~DevBufs() { for(void* q : p) hipFree(q); }
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
#define KT_TRY(expr) do { int rc_ = (expr); if(rc_) return rc_; } while(0)

void say(char* dst, size_t len, const std::string& s) { if(dst && len) { strncpy(dst, s.c_str(), len - 1); dst[len - 1] = 0; } }

}  // namespace

extern "C" {

// The kernels' constants, for tests that walk the round structure:
// 0 kPBlock  1 kP2StragPerBlock  2 kStragPerBlock  3 kGran  4 Ring<uint32_t>::kSlots  5 Ring<uint32_t>::kUnit  6 kTileBlock
// 7 items of a tile round (4-byte items)  8 the same for 8-byte items  9 kMaxTileBits  10 kBucketBits  11 kPTilePos
// 12 kG2Blocks  13 kTileQueueBytes
uint64_t jfkt_const(int which) {
  switch(which) {
    case 0: return kPBlock;
    case 1: return kP2StragPerBlock;
    case 2: return kStragPerBlock;
    case 3: return kGran;
    case 4: return Ring<uint32_t>::kSlots;
    case 5: return Ring<uint32_t>::kUnit;
    case 6: return kTileBlock;
    case 7: return 9216;
    case 8: return 4608;
    case 9: return kMaxTileBits;
    case 10: return kBucketBits;
    case 11: return kPTilePos;
    case 12: return kG2Blocks;
    case 13: return kTileQueueBytes;
  }
  return 0;
}

// The table's geometry as the kernels see it (TableGeom), for tests that restate make_item:
// 0 lsize_l 1 tile_bits 2 rem_bits 3 tag_bits 4 cnt_bits 5 slot32 6 hash_xs 7 nbytes 8 returning 9 part_ok 10 b1 11 b2
// 12 rest_shift 13 item32 14 lsize_g 15 canonical 16 tag_full (two-word keys: tile_bits + rem_bits) 17 key_bits (2k)
int jfkt_geom(jfgpu_table* t, uint64_t* out, uint32_t n) {
  if(!t || !out) return fail(JFGPU_E_INVALID, "null argument");
  const uint64_t v[18] = {t->g.lsize_l, t->g.tile_bits, t->g.rem_bits, t->g.tag_bits, t->g.cnt_bits, t->g.slot32, t->g.hash_xs, t->g.nbytes,
                          (uint64_t)t->returning, (uint64_t)t->part_ok, t->pg.b1, t->pg.b2, t->pg.rest_shift, (uint64_t)t->item32, t->g.lsize_g, t->g.canonical,
                          t->wide ? t->wt.W.tag_full : t->g.tile_bits + t->g.rem_bits, t->wide ? t->wt.W.g.key_bits : t->g.key_bits};
  for(uint32_t i = 0; i < n && i < 18; ++i) out[i] = v[i];
  return JFGPU_OK;
}

// ---- P2 alone ---------------------------------------------------------------------------------------------------------
// kernel: 0 p2_ring_roles_kernel<uint32_t, nv, RecordDirect, pd>, 1 p2_ring_kernel<RecordDirect> (kG2Blocks workgroups a
// bucket); then p1_stragglers_kernel<uint32_t, RecordDirect> over the launch's lists, as launch_p2_rings does.
// seg_items[s] / seg_off[s]: host arrays of segment s (n_items[s] items, n_off[s] offsets; sh[s] as SegList::sh).
// out: n_dest * cap items, in and out (the caller's sentinels come back where nothing was written).
// gcur: 2 * n_dest words out (cursors, then p2_ring_kernel's overflow notes), zero before the launch.
// rec: 3 * rec_cap words out, n_rec the number of DIRECT calls made (it may exceed rec_cap), ctr_direct what the kernels
// added to their direct counter, strag_n the lists' lengths (nbk, or kG2Blocks * nbk).
int jfkt_p2(jfgpu_table* t, int kernel, int nv, int pd, uint32_t b2e, uint32_t tag_bits, uint32_t n_seg,
            const void* const* seg_items, const uint64_t* n_items, const uint64_t* const* seg_off, const uint64_t* n_off, const uint32_t* sh,
            uint32_t cap, uint32_t bucket0, uint32_t nbk, uint32_t n_dest, uint32_t* out, uint32_t* gcur,
            uint64_t* rec, uint64_t rec_cap, uint64_t* n_rec, uint64_t* ctr_direct, uint32_t* strag_n, char* launched, size_t launched_len) {
  int rc = use(t); if(rc) return rc;
  if(!n_seg || n_seg > (uint32_t)kMaxSeg || !nbk || !cap) return fail(JFGPU_E_INVALID, "jfkt_p2: bad segment count, bucket count or capacity");
  if(b2e > 10 || (kernel == 0 && b2e != (nv == 2 ? 10u : 9u))) return fail(JFGPU_E_INVALID, "jfkt_p2: the host launches NV = 2 at 1024 destinations and NV = 1 at 512");
  if(kernel == 0 && (nv < 1 || nv > 2 || pd < 1 || pd > 3)) return fail(JFGPU_E_INVALID, "jfkt_p2: NV in {1, 2}, PD in {1, 2, 3}");
  if(kernel == 1 && b2e != 10) return fail(JFGPU_E_INVALID, "jfkt_p2: the shared-ring kernel is for 1024 destinations");
  if(((uint64_t)(bucket0 + nbk) << b2e) > n_dest) return fail(JFGPU_E_INVALID, "jfkt_p2: launched destinations beyond n_dest");
  if(cap % 4) return fail(JFGPU_E_INVALID, "jfkt_p2: regions start at multiples of 16 bytes");
  for(uint32_t s = 0; s < n_seg; ++s) {
    // what the kernels read must be inside what is allocated: offsets of every launched bucket within the items
    const uint64_t need = ((uint64_t)(bucket0 + nbk - 1) << sh[s]) + 2;
    if(sh[s] > 1 || n_off[s] < need) return fail(JFGPU_E_INVALID, "jfkt_p2: offsets do not cover the launched buckets");
    if(kernel == 1 && sh[s] != 1) return fail(JFGPU_E_INVALID, "jfkt_p2: the shared-ring kernel takes granule segments only");
    for(uint32_t j = bucket0; j < bucket0 + nbk; ++j) {
      const uint64_t a = seg_off[s][(size_t)j << sh[s]], b = seg_off[s][((size_t)j << sh[s]) + 1];
      if(a > b || b > n_items[s]) return fail(JFGPU_E_INVALID, "jfkt_p2: a bucket's range lies outside its segment");
      if(sh[s] == 1 && (a % 4)) return fail(JFGPU_E_INVALID, "jfkt_p2: a granule region starts at a multiple of 16 bytes");
    }
  }
  DevBufs D;
  SegList S; memset(&S, 0, sizeof S);
  S.n = n_seg;
  for(uint32_t s = 0; s < n_seg; ++s) {
    uint32_t* di; uint64_t* doff;
    KT_TRY(D.put(&di, (const uint32_t*)seg_items[s], (size_t)n_items[s], 4));      // (+ 16 bytes: nothing reads them, a wrong bound would)
    KT_TRY(D.put(&doff, seg_off[s], (size_t)n_off[s]));
    S.items[s] = di; S.off[s] = doff; S.sh[s] = sh[s];
  }
  const uint32_t n_lists = kernel == 0 ? nbk : kG2Blocks * nbk;
  uint32_t *d_out, *d_strag_n; unsigned int* d_gcur; uint64_t *d_strag, *d_rec; unsigned long long *d_nrec, *d_ctr;
  KT_TRY(D.put(&d_out, out, (size_t)n_dest * cap));
  KT_TRY(D.get(&d_gcur, 2 * (size_t)n_dest, 0));
  KT_TRY(D.get(&d_strag, (size_t)n_lists * kP2StragPerBlock, 0));
  KT_TRY(D.get(&d_strag_n, n_lists, 0));
  KT_TRY(D.get(&d_rec, 3 * (size_t)rec_cap, 0));
  KT_TRY(D.get(&d_nrec, 1, 0));
  KT_TRY(D.get(&d_ctr, 1, 0));
  const RecordDirect pd_{d_rec, d_nrec, rec_cap};
  const size_t lds = ((size_t)1 << b2e) * 128 + 128;                              // (launch_p2_rings)
  std::string name;
#define KT_P2R(NV, PD) do { KT_TRY(launch_lds(p2_ring_roles_kernel<uint32_t, NV, RecordDirect, PD>, dim3(nbk), dim3(kPBlock), lds, t->stream, pd_, b2e, tag_bits, S, cap, d_gcur, d_out, bucket0, d_strag, d_strag_n, d_ctr)); \
                            name = "p2_ring_roles_kernel<uint32_t," #NV ",RecordDirect," #PD ">"; } while(0)
  if(kernel == 0 && nv == 2) { if(pd == 1) KT_P2R(2, 1); else if(pd == 2) KT_P2R(2, 2); else KT_P2R(2, 3); }
  else if(kernel == 0) { if(pd == 1) KT_P2R(1, 1); else if(pd == 2) KT_P2R(1, 2); else KT_P2R(1, 3); }
#undef KT_P2R
  else {
    KT_TRY(launch_lds(p2_ring_kernel<RecordDirect>, dim3(kG2Blocks, nbk), dim3(kPBlock), lds, t->stream, pd_, b2e, tag_bits, S, cap, d_gcur, d_gcur + n_dest,
                       d_out, bucket0, (unsigned long long*)nullptr, d_strag, d_strag_n, d_ctr));
    name = "p2_ring_kernel<RecordDirect>";
  }
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL((p1_stragglers_kernel<uint32_t, RecordDirect>), dim3(t->n_cu), dim3(256), 0, t->stream, pd_, d_ctr, (const uint64_t*)d_strag, (const uint32_t*)d_strag_n,
                     n_lists, cap, d_gcur, (unsigned long long*)nullptr, d_out, kP2StragPerBlock);
  name += "+p1_stragglers_kernel<uint32_t,RecordDirect>";
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(t->stream));
  HIP_TRY(hipMemcpy(out, d_out, (size_t)n_dest * cap * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(gcur, d_gcur, 2 * (size_t)n_dest * 4, hipMemcpyDeviceToHost));
  if(rec_cap) HIP_TRY(hipMemcpy(rec, d_rec, 3 * (size_t)rec_cap * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(n_rec, d_nrec, 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ctr_direct, d_ctr, 8, hipMemcpyDeviceToHost));
  if(strag_n) HIP_TRY(hipMemcpy(strag_n, d_strag_n, (size_t)n_lists * 4, hipMemcpyDeviceToHost));
  say(launched, launched_len, name);
  return JFGPU_OK;
}

// ---- T alone ----------------------------------------------------------------------------------------------------------
// tile_rank_insert_kernel<ITEM, table's RETURNING, table's SLOT, tpb, kTileBlock, heavy, sample, holes> over n_units units
// from tile `tile0` of the table, one item array: unit u is items[off[u << sh] .. off[(u << sh) + 1]).  The instantiations
// are the host's (launch_tile_rank_variant): pairs of tiles for 4-byte items into 32-bit slots only, the hole-free one for
// the plain and the sampling kernel on such pairs only.  grid: workgroups (0: one per unit).
int jfkt_tile(jfgpu_table* t, int tpb, int heavy, int sample, int holes, uint32_t item_bytes, const void* items, uint64_t n_items,
              const uint64_t* off, uint64_t n_off, uint32_t sh, uint64_t tile0, uint32_t n_units, uint32_t grid, char* launched, size_t launched_len) {
  int rc = use(t); if(rc) return rc;
  if(t->wide || t->nword || t->g.tile_bits != kMaxTileBits) return fail(JFGPU_E_INVALID, "jfkt_tile: one-word keys, full-size tiles");
  if((tpb != 1 && tpb != 2) || (item_bytes != 4 && item_bytes != 8) || sh > 1 || !n_units) return fail(JFGPU_E_INVALID, "jfkt_tile: bad arguments");
  if(tpb == 2 && !(item_bytes == 4 && t->g.slot32)) return fail(JFGPU_E_INVALID, "jfkt_tile: pairs of tiles take 4-byte items into 32-bit slots");
  if(heavy && sample) return fail(JFGPU_E_INVALID, "jfkt_tile: the sampling kernel is the plain one");
  if(!holes && !(tpb == 2 && !heavy)) return fail(JFGPU_E_INVALID, "jfkt_tile: the hole-free instantiation is the plain kernel's on pairs of tiles");
  if(tile0 + (uint64_t)tpb * n_units > n_tiles_of(t)) return fail(JFGPU_E_INVALID, "jfkt_tile: units beyond the table");
  if(n_off < (((uint64_t)n_units - 1) << sh) + 2) return fail(JFGPU_E_INVALID, "jfkt_tile: offsets do not cover the units");
  for(uint32_t u = 0; u < n_units; ++u) {
    const uint64_t a = off[(size_t)u << sh], b = off[((size_t)u << sh) + 1];
    if(a > b || b > n_items) return fail(JFGPU_E_INVALID, "jfkt_tile: a unit's range lies outside the items");
  }
  DevBufs D;
  uint8_t* d_items; uint64_t* d_off;
  KT_TRY(D.put(&d_items, (const uint8_t*)items, (size_t)n_items * item_bytes, 16));
  KT_TRY(D.put(&d_off, off, (size_t)n_off));
  SegList S; memset(&S, 0, sizeof S);
  S.n = 1; S.items[0] = d_items; S.off[0] = d_off; S.sh[0] = sh; S.dense[0] = holes ? 0 : 1;
  const dim3 g(grid ? std::min(grid, n_units) : n_units), block(kTileBlock);
  const size_t lds = tile_rank_lds(t->g.slot32 ? 4 : 8, t->g.tile_bits, tpb);
  const bool rt = t->returning;
  std::string name;
#define KT_T(I, SL, P, H, M, HL) do { \
    if(rt) KT_TRY(launch_lds(tile_rank_insert_kernel<I, true, SL, P, kTileBlock, H, M, HL>, g, block, lds, t->stream, t->dt, S, tile0, n_units)); \
    else   KT_TRY(launch_lds(tile_rank_insert_kernel<I, false, SL, P, kTileBlock, H, M, HL>, g, block, lds, t->stream, t->dt, S, tile0, n_units)); \
    name = std::string("tile_rank_insert_kernel<" #I ",") + (rt ? "true" : "false") + "," #SL "," #P ",kTileBlock," #H "," #M "," #HL ">"; } while(0)
#define KT_TV(I, SL, P) do { if(heavy) KT_T(I, SL, P, true, false, true); else if(sample) KT_T(I, SL, P, false, true, true); else KT_T(I, SL, P, false, false, true); } while(0)
  if(!holes) { if(sample) KT_T(uint32_t, unsigned int, 2, false, true, false); else KT_T(uint32_t, unsigned int, 2, false, false, false); }
  else if(item_bytes == 4 && t->g.slot32 && tpb == 2) KT_TV(uint32_t, unsigned int, 2);
  else if(item_bytes == 4 && t->g.slot32) KT_TV(uint32_t, unsigned int, 1);
  else if(item_bytes == 4) KT_TV(uint32_t, unsigned long long, 1);
  else if(t->g.slot32) KT_TV(uint64_t, unsigned int, 1);
  else KT_TV(uint64_t, unsigned long long, 1);
#undef KT_TV
#undef KT_T
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(t->stream));
  t->pristine = false;
  say(launched, launched_len, name);
  return JFGPU_OK;
}

// ---- P1 alone ---------------------------------------------------------------------------------------------------------
// p1_ring_kernel<uint32_t, false, NB, CANON, RecordDirect> over bases[lo, hi) (a contract buffer: its base 16-byte
// aligned) on the table's descriptor with 2^b1 buckets (PartGeom set here: rest_shift = lsize_l - b1), `grid` workgroups.
// variant: 0 the run-time byte-table hash (NB = 0, CANON = 2); 1 six key bytes compiled in (NB = 6, CANON the table's);
// 2 the xor-shift matrix in registers (NB = kHashXSLow, CANON = 2; the table's matrix must be that one).
// Neither p1_stragglers_kernel nor granule_finish_kernel runs: the lists come back as the kernel left them.
// out: (2^b1 + 1) * cap items in and out (one region behind the last bucket's: a guard); gcur: 2 * 2^b1 words out; tot: 2^b1 out; strag: grid * kStragPerBlock entries out,
// strag_n: grid; rec / n_rec as in jfkt_p2; ctr[2]: what the kernel added to the table's k-mer counter and to its direct counter.
int jfkt_p1(jfgpu_table* t, int variant, uint32_t b1, const uint8_t* bases, uint64_t n_bases, int64_t lo, int64_t hi, uint32_t cap, uint32_t grid,
            uint32_t* out, uint32_t* gcur, uint64_t* tot, uint64_t* strag, uint32_t* strag_n, uint64_t* rec, uint64_t rec_cap, uint64_t* n_rec,
            uint64_t* ctr, char* launched, size_t launched_len) {
  int rc = use(t); if(rc) return rc;
  if(t->wide || t->nword) return fail(JFGPU_E_INVALID, "jfkt_p1: one-word keys");
  if(b1 < 1 || b1 > 10 || b1 > t->g.lsize_l || !grid || grid > 64) return fail(JFGPU_E_INVALID, "jfkt_p1: 1 <= b1 <= 10, 1 <= grid <= 64");
  if(lo < 0 || hi < lo || (uint64_t)hi > n_bases) return fail(JFGPU_E_INVALID, "jfkt_p1: [lo, hi) outside the buffer");
  if(cap % kGran || !cap) return fail(JFGPU_E_INVALID, "jfkt_p1: regions are whole reservations");
  PartGeom P;
  P.b1 = b1; P.b2 = t->g.lsize_l - t->g.tile_bits > b1 ? t->g.lsize_l - t->g.tile_bits - b1 : 0;
  P.rest_shift = t->g.lsize_l - b1; P.item_bits = P.rest_shift + t->g.rem_bits;
  if(P.item_bits > 32) return fail(JFGPU_E_INVALID, "jfkt_p1: the geometry's items do not fit 32 bits");
  if(variant == 1 && t->g.nbytes != 6) return fail(JFGPU_E_INVALID, "jfkt_p1: NB = 6 needs keys of six bytes");
  if(variant == 2 && !t->g.hash_xs) return fail(JFGPU_E_INVALID, "jfkt_p1: the table's matrix is not the xor-shift one");
  if(variant == 2 && t->g.lsize_g > 32) return fail(JFGPU_E_INVALID, "jfkt_p1: kHashXSLow is for positions of at most 32 bits");
  const uint32_t nb = 1u << b1;
  DevBufs D;
  uint8_t* d_bases; uint32_t *d_out, *d_strag_n; unsigned int* d_gcur; unsigned long long *d_tot, *d_nrec; uint64_t *d_strag, *d_rec;
  KT_TRY(D.put(&d_bases, bases, (size_t)n_bases, 32));
  KT_TRY(D.put(&d_out, out, ((size_t)nb + 1) * cap));
  KT_TRY(D.get(&d_gcur, 2 * (size_t)nb, 0));
  KT_TRY(D.get(&d_tot, nb, 0));
  KT_TRY(D.get(&d_strag, (size_t)grid * kStragPerBlock, 0));
  KT_TRY(D.get(&d_strag_n, grid, 0));
  KT_TRY(D.get(&d_rec, 3 * (size_t)rec_cap, 0));
  KT_TRY(D.get(&d_nrec, 1, 0));
  uint64_t c0[CTR_COUNT], c1[CTR_COUNT];
  KT_TRY(read_counters(t, c0));
  const RecordDirect od{d_rec, d_nrec, rec_cap};
  const size_t lds = (size_t)nb * 128 + 128;                                      // (part_ingest)
  std::string name;
#define KT_P1(N, CN) do { KT_TRY(launch_lds(p1_ring_kernel<uint32_t, false, N, CN, RecordDirect>, dim3(grid), dim3(kPBlock), lds, t->stream, t->dt, od, P, (const uint8_t*)d_bases, lo, hi, cap, d_gcur, d_tot, d_out, d_strag, d_strag_n)); \
                          name = "p1_ring_kernel<uint32_t,false," #N "," #CN ",RecordDirect>"; } while(0)
  if(variant == 0) KT_P1(0, 2);
  else if(variant == 1) { if(t->g.canonical) KT_P1(6, 1); else KT_P1(6, 0); }
  else KT_P1(kHashXSLow, 2);
#undef KT_P1
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(t->stream));
  KT_TRY(read_counters(t, c1));
  HIP_TRY(hipMemcpy(out, d_out, ((size_t)nb + 1) * cap * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(gcur, d_gcur, 2 * (size_t)nb * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(tot, d_tot, (size_t)nb * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(strag, d_strag, (size_t)grid * kStragPerBlock * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(strag_n, d_strag_n, (size_t)grid * 4, hipMemcpyDeviceToHost));
  if(rec_cap) HIP_TRY(hipMemcpy(rec, d_rec, 3 * (size_t)rec_cap * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(n_rec, d_nrec, 8, hipMemcpyDeviceToHost));
  if(ctr) { ctr[0] = c1[CTR_MERS] - c0[CTR_MERS]; ctr[1] = c1[CTR_DIRECT] - c0[CTR_DIRECT]; }
  say(launched, launched_len, name);
  return JFGPU_OK;
}

// ---- the sort-based P2 alone ------------------------------------------------------------------------------------------
// scheme 0 (single pass): p2_granule_kernel<ITEM, RecordDirectT<ITEM>, PER> with (ITEM, PER) = (uint32_t, kP2PairPer),
// (uint64_t, kP2MidPer), (u128, kP2WidePer), grid (4, nbk), then granule_finish_kernel over all n_dest destinations -- or,
// with fr_nd > 0, granule_finish_range_kernel over destinations [fr_d0, fr_d0 + fr_nd).
// scheme 1 (exact): p2_kernel<ITEM, false>, scan_matrix_kernel, p2_scatter_sorted_kernel<ITEM, PER> with the host's PER
// (28 for pairs of tiles, else 16 / 14 / 7), 32 workgroups a bucket; base[q]: where bucket q's items start in out.
// Items of 16 bytes are pairs of 64-bit words, low word first.  Segments as in jfkt_p2.
// out: n_out items in and out (scheme 0: n_out = n_dest * cap).  gcur: 2 * n_dest words out (scheme 0).  off2: 2 * n_dest
// words in and out (scheme 0).  goff: n_dest + 1 words in and out (scheme 1).  rec: 3 * rec_cap words (destination, low, high).
int jfkt_p2_sort(jfgpu_table* t, int scheme, uint32_t item_bytes, int pair, uint32_t b2e, uint32_t tag_bits, uint32_t n_seg,
                 const void* const* seg_items, const uint64_t* n_items, const uint64_t* const* seg_off, const uint64_t* n_off, const uint32_t* sh,
                 uint32_t cap, uint32_t bucket0, uint32_t nbk, uint32_t n_dest, void* out, uint64_t n_out, uint32_t* gcur, uint64_t* off2,
                 uint32_t fr_d0, uint32_t fr_nd, const uint64_t* base, uint64_t* goff,
                 uint64_t* rec, uint64_t rec_cap, uint64_t* n_rec, uint64_t* ctr_direct, char* launched, size_t launched_len) {
  int rc = use(t); if(rc) return rc;
  if(scheme < 0 || scheme > 1 || (item_bytes != 4 && item_bytes != 8 && item_bytes != 16)) return fail(JFGPU_E_INVALID, "jfkt_p2_sort: scheme 0 or 1, items of 4, 8 or 16 bytes");
  if(!n_seg || n_seg > (uint32_t)kMaxSeg || !nbk) return fail(JFGPU_E_INVALID, "jfkt_p2_sort: bad segment or bucket count");
  if(b2e > (scheme == 0 ? 10u : 11u)) return fail(JFGPU_E_INVALID, "jfkt_p2_sort: the single-pass kernel places one destination per thread (at most 1024), the exact ones take 2048");
  if(tag_bits + b2e > 8 * item_bytes || tag_bits >= 8 * item_bytes) return fail(JFGPU_E_INVALID, "jfkt_p2_sort: the sub-bucket lies outside the item");
  if(pair && item_bytes != 4) return fail(JFGPU_E_INVALID, "jfkt_p2_sort: pairs of tiles take 4-byte items");
  if(((uint64_t)(bucket0 + nbk) << b2e) > n_dest) return fail(JFGPU_E_INVALID, "jfkt_p2_sort: launched destinations beyond n_dest");
  if(scheme == 0 && (!cap || cap % kGran || (uint64_t)n_dest * cap != n_out)) return fail(JFGPU_E_INVALID, "jfkt_p2_sort: regions are whole reservations, out is n_dest regions");
  if(scheme == 0 && fr_nd && (uint64_t)fr_d0 + fr_nd > n_dest) return fail(JFGPU_E_INVALID, "jfkt_p2_sort: the finish range lies outside the destinations");
  for(uint32_t s = 0; s < n_seg; ++s) {
    const uint64_t need = ((uint64_t)(bucket0 + nbk - 1) << sh[s]) + 2;
    if(sh[s] > 1 || n_off[s] < need) return fail(JFGPU_E_INVALID, "jfkt_p2_sort: offsets do not cover the launched buckets");
    for(uint32_t j = bucket0; j < bucket0 + nbk; ++j) {
      const uint64_t a = seg_off[s][(size_t)j << sh[s]], b = seg_off[s][((size_t)j << sh[s]) + 1];
      if(a > b || b > n_items[s]) return fail(JFGPU_E_INVALID, "jfkt_p2_sort: a bucket's range lies outside its segment");
    }
  }
  if(scheme == 1) {      // every launched bucket's items inside out
    if(!base) return fail(JFGPU_E_INVALID, "jfkt_p2_sort: the exact scheme needs base");
    for(uint32_t j = bucket0; j < bucket0 + nbk; ++j) {
      uint64_t n = 0;
      for(uint32_t s = 0; s < n_seg; ++s) {                 // (what the kernels store: every entry, but for a granule segment's holes)
        const uint64_t a = seg_off[s][(size_t)j << sh[s]], b = seg_off[s][((size_t)j << sh[s]) + 1];
        n += b - a;
        const uint8_t* e = (const uint8_t*)seg_items[s];
        for(uint64_t i = a; sh[s] && i < b; ++i) {
          bool hole = true;
          for(uint32_t c = 0; c < item_bytes; ++c) hole = hole && e[i * item_bytes + c] == 0xFF;
          n -= hole;
        }
      }
      if(n >> 32 || base[j] + n > n_out) return fail(JFGPU_E_INVALID, "jfkt_p2_sort: a bucket's items do not fit out behind base");
    }
  }
  DevBufs D;
  SegList S; memset(&S, 0, sizeof S);
  S.n = n_seg;
  for(uint32_t s = 0; s < n_seg; ++s) {
    uint8_t* di; uint64_t* doff;
    KT_TRY(D.put(&di, (const uint8_t*)seg_items[s], (size_t)n_items[s] * item_bytes, 16));
    KT_TRY(D.put(&doff, seg_off[s], (size_t)n_off[s]));
    S.items[s] = di; S.off[s] = doff; S.sh[s] = sh[s];
  }
  uint8_t* d_out; uint64_t* d_rec; unsigned long long *d_nrec, *d_ctr;
  KT_TRY(D.put(&d_out, (const uint8_t*)out, (size_t)n_out * item_bytes));
  KT_TRY(D.get(&d_rec, 3 * (size_t)rec_cap, 0));
  KT_TRY(D.get(&d_nrec, 1, 0));
  KT_TRY(D.get(&d_ctr, 1, 0));
  const dim3 block(kPBlock);
  std::string name;
  if(scheme == 0) {
    unsigned int* d_gcur; uint64_t* d_off2;
    KT_TRY(D.get(&d_gcur, 2 * (size_t)n_dest, 0));
    KT_TRY(D.put(&d_off2, off2, 2 * (size_t)n_dest));
    const dim3 g1p(4, nbk);
#define KT_G(I, PER) do { \
      const RecordDirectT<I> rd{d_rec, d_nrec, rec_cap, d_ctr, b2e, tag_bits}; \
      const size_t lds = (size_t)kPBlock * PER * sizeof(I); \
      KT_TRY(launch_lds(p2_granule_kernel<I, RecordDirectT<I>, PER>, g1p, block, lds, t->stream, rd, b2e, tag_bits, S, cap, d_gcur, d_gcur + n_dest, (I*)d_out, bucket0, (unsigned long long*)nullptr, 0xFFFFFFFFu)); \
      name = "p2_granule_kernel<" #I ",RecordDirectT<" #I ">," #PER ">"; } while(0)
    if(item_bytes == 4) KT_G(uint32_t, kP2PairPer); else if(item_bytes == 8) KT_G(uint64_t, kP2MidPer); else KT_G(u128, kP2WidePer);
#undef KT_G
    HIP_TRY(hipGetLastError());
    if(fr_nd) { hipLaunchKernelGGL(granule_finish_range_kernel, dim3(256), dim3(256), 0, t->stream, d_gcur, cap, n_dest, d_off2, fr_d0, fr_nd); name += "+granule_finish_range_kernel"; }
    else { hipLaunchKernelGGL(granule_finish_kernel, dim3(1024), dim3(256), 0, t->stream, d_gcur, cap, n_dest, d_off2); name += "+granule_finish_kernel"; }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(t->stream));
    HIP_TRY(hipMemcpy(gcur, d_gcur, 2 * (size_t)n_dest * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(off2, d_off2, 2 * (size_t)n_dest * 8, hipMemcpyDeviceToHost));
  } else {
    const int g2 = 32;
    const uint32_t nb1 = bucket0 + nbk, nb2e = 1u << b2e;
    uint32_t* d_M2; uint64_t *d_goff, *d_base;
    KT_TRY(D.get(&d_M2, (size_t)nb1 * g2 * nb2e, 0));
    KT_TRY(D.put(&d_goff, goff, (size_t)n_dest + 1));
    KT_TRY(D.put(&d_base, base, nb1));
    PartGeom pg2; memset(&pg2, 0, sizeof pg2);
    pg2.b2 = b2e;
    const dim3 grid(g2, nbk);
#define KT_X(I, PER) do { \
      hipLaunchKernelGGL((p2_kernel<I, false>), grid, block, 0, t->stream, pg2, tag_bits, S, d_M2, (const uint64_t*)d_goff, (I*)d_out, bucket0); \
      hipLaunchKernelGGL(scan_matrix_kernel, dim3(nbk), dim3(1024), 0, t->stream, d_M2, (uint32_t)g2, nb2e, (const uint64_t*)d_base, d_goff, bucket0); \
      KT_TRY(launch_lds(p2_scatter_sorted_kernel<I, PER>, grid, block, (size_t)kPBlock * PER * sizeof(I), t->stream, pg2, tag_bits, S, (const uint32_t*)d_M2, (const uint64_t*)d_goff, (I*)d_out, bucket0)); \
      name = "p2_kernel<" #I ",false>+scan_matrix_kernel+p2_scatter_sorted_kernel<" #I "," #PER ">"; } while(0)
    if(item_bytes == 4 && pair) KT_X(uint32_t, kP2PairPer); else if(item_bytes == 4) KT_X(uint32_t, 16); else if(item_bytes == 8) KT_X(uint64_t, 14); else KT_X(u128, 7);
#undef KT_X
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(t->stream));
    HIP_TRY(hipMemcpy(goff, d_goff, ((size_t)n_dest + 1) * 8, hipMemcpyDeviceToHost));
  }
  HIP_TRY(hipMemcpy(out, d_out, (size_t)n_out * item_bytes, hipMemcpyDeviceToHost));
  if(rec_cap) HIP_TRY(hipMemcpy(rec, d_rec, 3 * (size_t)rec_cap * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(n_rec, d_nrec, 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ctr_direct, d_ctr, 8, hipMemcpyDeviceToHost));
  say(launched, launched_len, name);
  return JFGPU_OK;
}

// ---- P1w alone --------------------------------------------------------------------------------------------------------
// p1_wide_granule_kernel<table's RETURNING, false, XS> (XS: the table's matrix is the xor-shift one) over bases[lo, hi) with
// 2^b1 buckets, `grid` workgroups.  PartGeom as in jfkt_p1, b2 = what is left of the tile index.  This kernel's overflow
// is not a template argument: what a region cannot take is claimed in the table itself (wide_item_direct), which needs
// the buckets to be groups of whole tiles -- so b1 beyond the table's tile-index bits is taken only with regions that
// cannot overflow (cap >= hi - lo + grid * kGran).
// out: (2^b1 + 1) * cap items of two words in and out (the last region is a guard); gcur: 2 * 2^b1 words out; tot: 2^b1 out;
// ctr[2]: what the kernel added to the table's k-mer counter and to its direct counter.
int jfkt_p1_wide(jfgpu_table* t, uint32_t b1, const uint8_t* bases, uint64_t n_bases, int64_t lo, int64_t hi, uint32_t cap, uint32_t grid,
                 uint64_t* out, uint32_t* gcur, uint64_t* tot, uint64_t* ctr, char* launched, size_t launched_len) {
  int rc = use(t); if(rc) return rc;
  if(!t->wide || !t->item128 || t->wt.bloom.data) return fail(JFGPU_E_INVALID, "jfkt_p1_wide: two-word keys with the partitioned geometry, no filter");
  if(b1 > 10 || b1 > t->g.lsize_l || !grid || grid > 64) return fail(JFGPU_E_INVALID, "jfkt_p1_wide: 0 <= b1 <= 10, 1 <= grid <= 64");
  if(lo < 0 || hi < lo || (uint64_t)hi > n_bases) return fail(JFGPU_E_INVALID, "jfkt_p1_wide: [lo, hi) outside the buffer");
  if(cap % kGran || !cap) return fail(JFGPU_E_INVALID, "jfkt_p1_wide: regions are whole reservations");
  const uint32_t tbits = t->g.lsize_l - t->g.tile_bits;
  if(b1 > tbits && (uint64_t)cap < (uint64_t)(hi - lo) + (uint64_t)grid * kGran) return fail(JFGPU_E_INVALID, "jfkt_p1_wide: buckets smaller than a tile need regions that cannot overflow");
  PartGeom P;
  P.b1 = b1; P.b2 = tbits > b1 ? tbits - b1 : 0;
  P.rest_shift = t->g.lsize_l - b1; P.item_bits = P.rest_shift + t->g.rem_bits;
  if(P.item_bits > 128) return fail(JFGPU_E_INVALID, "jfkt_p1_wide: the geometry's items do not fit 128 bits");
  const uint32_t nb = 1u << b1;
  DevBufs D;
  uint8_t* d_bases; uint64_t* d_out; unsigned int* d_gcur; unsigned long long* d_tot;
  KT_TRY(D.put(&d_bases, bases, (size_t)n_bases, 32));
  KT_TRY(D.put(&d_out, out, ((size_t)nb + 1) * cap * 2));
  KT_TRY(D.get(&d_gcur, 2 * (size_t)nb, 0));
  KT_TRY(D.get(&d_tot, nb, 0));
  uint64_t c0[CTR_COUNT], c1[CTR_COUNT];
  KT_TRY(read_counters(t, c0));
  const size_t wlds = (size_t)kWideChunk * 18 + (size_t)t->g.nbytes * 2048;         // (part_ingest)
  const bool xs = t->g.hash_xs != 0;
  std::string name;
#define KT_PW(RT, X) do { KT_TRY(launch_lds(p1_wide_granule_kernel<RT, false, X>, dim3(grid), dim3(kPBlock), wlds, t->stream, t->wt, P, (const uint8_t*)d_bases, lo, hi, cap, d_gcur, d_tot, (u128*)d_out)); \
                          name = "p1_wide_granule_kernel<" #RT ",false," #X ">"; } while(0)
  if(xs) { if(t->returning) KT_PW(true, true); else KT_PW(false, true); }
  else { if(t->returning) KT_PW(true, false); else KT_PW(false, false); }
#undef KT_PW
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(t->stream));
  t->pristine = false;
  KT_TRY(read_counters(t, c1));
  HIP_TRY(hipMemcpy(out, d_out, ((size_t)nb + 1) * cap * 16, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(gcur, d_gcur, 2 * (size_t)nb * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(tot, d_tot, (size_t)nb * 8, hipMemcpyDeviceToHost));
  if(ctr) { ctr[0] = c1[CTR_MERS] - c0[CTR_MERS]; ctr[1] = c1[CTR_DIRECT] - c0[CTR_DIRECT]; }
  say(launched, launched_len, name);
  return JFGPU_OK;
}

// ---- Tw alone ---------------------------------------------------------------------------------------------------------
// kernel 0: tile_insert_wide_kernel<table's RETURNING> over n_units tiles from tile0, 1 to 3 segments;
// kernel 1: tile_insert_wide_pipe_kernel<table's RETURNING>, exactly one segment;
// kernel 2: items_direct_wide_kernel<table's RETURNING> over one granule batch of the table's own P1 geometry: segment 0
//           holds 2^b1 regions of `cap` items and their (begin, end) pairs.
// Unit u of segment s is items[off[u << sh] .. off[(u << sh) + 1]) as in jfkt_tile; items are pairs of words, low first.
int jfkt_tile_wide(jfgpu_table* t, int kernel, uint32_t n_seg, const void* const* seg_items, const uint64_t* n_items, const uint64_t* const* seg_off,
                   const uint64_t* n_off, const uint32_t* sh, uint64_t tile0, uint32_t n_units, uint32_t grid, uint64_t cap, char* launched, size_t launched_len) {
  int rc = use(t); if(rc) return rc;
  if(!t->wide || !t->item128 || t->g.tile_bits != kMaxTileBits || !t->wt.dirty) return fail(JFGPU_E_INVALID, "jfkt_tile_wide: two-word keys, full-size tiles");
  if(kernel < 0 || kernel > 2 || !n_seg || n_seg > 3 || (kernel != 0 && n_seg != 1) || !grid) return fail(JFGPU_E_INVALID, "jfkt_tile_wide: bad kernel, segment count or grid");
  if(kernel == 2) {
    const uint64_t nb = 1ull << t->pg.b1;
    if(!cap || sh[0] != 1 || n_items[0] != nb * cap || n_off[0] < 2 * nb) return fail(JFGPU_E_INVALID, "jfkt_tile_wide: a granule batch is 2^b1 regions of cap items");
    for(uint64_t b = 0; b < nb; ++b) if(seg_off[0][2 * b + 1] > (b + 1) * cap) return fail(JFGPU_E_INVALID, "jfkt_tile_wide: a region ends beyond itself");
  } else {
    if(!n_units || tile0 + n_units > n_tiles_of(t)) return fail(JFGPU_E_INVALID, "jfkt_tile_wide: units beyond the table");
    for(uint32_t s = 0; s < n_seg; ++s) {
      if(sh[s] > 1 || n_off[s] < (((uint64_t)n_units - 1) << sh[s]) + 2) return fail(JFGPU_E_INVALID, "jfkt_tile_wide: offsets do not cover the units");
      for(uint32_t u = 0; u < n_units; ++u) {
        const uint64_t a = seg_off[s][(size_t)u << sh[s]], b = seg_off[s][((size_t)u << sh[s]) + 1];
        if(a > b || b > n_items[s]) return fail(JFGPU_E_INVALID, "jfkt_tile_wide: a unit's range lies outside the items");
      }
    }
  }
  DevBufs D;
  SegList S; memset(&S, 0, sizeof S);
  S.n = n_seg;
  for(uint32_t s = 0; s < n_seg; ++s) {
    uint64_t *di, *doff;
    KT_TRY(D.put(&di, (const uint64_t*)seg_items[s], (size_t)n_items[s] * 2, 2));
    KT_TRY(D.put(&doff, seg_off[s], (size_t)n_off[s]));
    S.items[s] = di; S.off[s] = doff; S.sh[s] = sh[s];
  }
  const size_t tile_lds = (size_t)16 << t->g.tile_bits;                             // (part_flush_t)
  const bool rt = t->returning;
  const char* r = rt ? "true" : "false";
  std::string name;
  if(kernel == 0) {
    const dim3 g(std::min(grid, n_units)), block(kPBlock);
    if(rt) KT_TRY(launch_lds(tile_insert_wide_kernel<true>, g, block, tile_lds, t->stream, t->wt, S, tile0, n_units));
    else   KT_TRY(launch_lds(tile_insert_wide_kernel<false>, g, block, tile_lds, t->stream, t->wt, S, tile0, n_units));
    name = std::string("tile_insert_wide_kernel<") + r + ">";
  } else if(kernel == 1) {
    const dim3 g(std::min(grid, n_units)), block(kPBlock);
    if(rt) KT_TRY(launch_lds(tile_insert_wide_pipe_kernel<true>, g, block, tile_lds, t->stream, t->wt, S, tile0, n_units));
    else   KT_TRY(launch_lds(tile_insert_wide_pipe_kernel<false>, g, block, tile_lds, t->stream, t->wt, S, tile0, n_units));
    name = std::string("tile_insert_wide_pipe_kernel<") + r + ">";
  } else {
    const dim3 g(grid), block(kBlock);
    if(rt) hipLaunchKernelGGL(items_direct_wide_kernel<true>, g, block, 0, t->stream, t->wt, t->pg, (const u128*)S.items[0], S.off[0], cap);
    else   hipLaunchKernelGGL(items_direct_wide_kernel<false>, g, block, 0, t->stream, t->wt, t->pg, (const u128*)S.items[0], S.off[0], cap);
    name = std::string("items_direct_wide_kernel<") + r + ">";
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(t->stream));
  t->pristine = false;
  say(launched, launched_len, name);
  return JFGPU_OK;
}

}  // extern "C"

// ---- the partitioned Bloom insert (kernels_bloom_part.hip.hpp) ----------------------------------------------------------
// Every entry point takes a counter made by THIS library's jfgpu_bc_create: kind 0, part_ok (whole segments are allocated,
// so Tb may load and store them), left in mode 1 so that the engine itself launches nothing partitioned, nothing pending.
// The BloomPart is the caller's: n_seg must be the filter's own and 2^(b1 + b2) buckets x sub-buckets must cover it.  The
// filter's bytes go in and come out through jfgpu_bc_load / jfgpu_bc_read.  The functors are the product's own (BloomDirect,
// BloomRingDirect, BloomP1RingDirect): what they do IS the output here, a side effect on the filter.
namespace {

int kt_bloom_use(jfgpu_bloom* b, const BloomPart& BP, const char* who) {
  int rc = use_b(b); if(rc) return rc;
  if(b->kind != 0 || !b->part_ok || b->mode != 1 || !b->pending.empty() || b->wide || b->nword)
    return fail(JFGPU_E_INVALID, std::string(who) + ": a Bloom counter of one-word keys with whole segments, in mode 1, nothing pending");
  if(BP.n_seg != b->bp.n_seg || BP.b1 > 10 || BP.b2 > 11 || ((uint64_t)1 << (BP.b1 + BP.b2)) < BP.n_seg)
    return fail(JFGPU_E_INVALID, std::string(who) + ": n_seg is the filter's own, b1 <= 10, b2 <= 11, n_seg <= 2^(b1 + b2)");
  return JFGPU_OK;
}

// a cell update the kernels may be given: digit below five, (with `bucket`) a segment of the filter
bool kt_bloom_item_ok(const BloomPart& BP, uint32_t bucket, uint32_t item) {
  const uint64_t sub = item >> kBloomItemLow;
  return (item & 7u) <= 4u && sub < ((uint64_t)1 << BP.b2) && (((uint64_t)bucket << BP.b2) | sub) < BP.n_seg;
}

}  // namespace

extern "C" {

// 0 kBloomSegBits  1 kBloomItemLow  2 kBloomPer  3 kBloomRingBytes  4 kP2PairPer  5 kGranMaxB
uint64_t jfkt_bloom_const(int which) {
  switch(which) {
    case 0: return kBloomSegBits;
    case 1: return kBloomItemLow;
    case 2: return kBloomPer;
    case 3: return kBloomRingBytes;
    case 4: return kP2PairPer;
    case 5: return kGranMaxB;
  }
  return 0;
}

// ---- P1b alone --------------------------------------------------------------------------------------------------------
// family 0: p1_bloom_granule_kernel<NB> (per = 10); 1: p1_bloom_granule2_kernel<NB> (per = 5); 2: p1_bloom_ring_kernel<NB, per>
// with (NB, per) in {0, 6, 8} x {10} and {0, 8} x {5}, at most 512 buckets -- the instantiations bloom_ingest launches, with
// its dynamic-LDS sizes -- over bases[lo, hi) (a contract buffer, its base 16-byte aligned), `grid` workgroups.
// run_stragglers (ring family): p1_stragglers_kernel<uint32_t, BloomP1RingDirect> over the lists afterwards, as bloom_ingest does.
// out: (2^b1 + 1) * cap items in and out (the last region is a guard); gcur: 2 * 2^b1 words out (cursors, overflow notes);
// tot: 2^b1; strag: grid * kStragPerBlock entries and strag_n: grid, as the P1b kernel left them (ring family; else zero);
// mers: what the launch added to the counter's k-mer count.
int jfkt_bloom_p1(jfgpu_bloom* b, int family, int nbt, int per, uint32_t b1, uint32_t b2, uint32_t n_seg, const uint8_t* bases, uint64_t n_bases,
                  int64_t lo, int64_t hi, uint32_t cap, uint32_t grid, int run_stragglers, uint32_t* out, uint32_t* gcur, uint64_t* tot,
                  uint64_t* strag, uint32_t* strag_n, uint64_t* mers, char* launched, size_t launched_len) {
  const BloomPart BP{b1, b2, n_seg, 0};
  int rc = kt_bloom_use(b, BP, "jfkt_bloom_p1"); if(rc) return rc;
  if(family < 0 || family > 2 || !grid || grid > 64) return fail(JFGPU_E_INVALID, "jfkt_bloom_p1: family 0, 1 or 2, 1 <= grid <= 64");
  if(lo < 0 || hi < lo || (uint64_t)hi > n_bases) return fail(JFGPU_E_INVALID, "jfkt_bloom_p1: [lo, hi) outside the buffer");
  if(cap % kGran || !cap) return fail(JFGPU_E_INVALID, "jfkt_bloom_p1: regions are whole reservations");
  if((nbt != 0 && nbt != 6 && nbt != 8) || (nbt && (uint32_t)nbt != b->g.nbytes) || b->g.nbytes > 8) return fail(JFGPU_E_INVALID, "jfkt_bloom_p1: NB is 0 or the key's bytes (6 or 8)");
  if((family == 0 && per != kBloomPer) || (family == 1 && per != 5)) return fail(JFGPU_E_INVALID, "jfkt_bloom_p1: the sort-based kernels take 10 (byte tables) and 5 (nibble tables) cells a round");
  if(family == 2 && !((per == 10) || (per == 5 && nbt != 6))) return fail(JFGPU_E_INVALID, "jfkt_bloom_p1: the host launches rings with (NB, PER) in {0, 6, 8} x {10} and {0, 8} x {5}");
  if(family == 2 && b1 > 9) return fail(JFGPU_E_INVALID, "jfkt_bloom_p1: the ring kernel takes at most 512 buckets");
  if(run_stragglers && family != 2) return fail(JFGPU_E_INVALID, "jfkt_bloom_p1: the sort-based kernels leave no lists");
  const uint32_t nb = 1u << b1;
  DevBufs D;
  uint8_t* d_bases; uint32_t *d_out, *d_strag_n; unsigned int* d_gcur; unsigned long long* d_tot; uint64_t* d_strag;
  KT_TRY(D.put(&d_bases, bases, (size_t)n_bases, 32));
  KT_TRY(D.put(&d_out, out, ((size_t)nb + 1) * cap));
  KT_TRY(D.get(&d_gcur, 2 * (size_t)nb, 0));
  KT_TRY(D.get(&d_tot, nb, 0));
  KT_TRY(D.get(&d_strag, (size_t)grid * kStragPerBlock, 0));
  KT_TRY(D.get(&d_strag_n, grid, 0));
  unsigned long long m0 = 0, m1 = 0;
  HIP_TRY(hipMemcpy(&m0, b->d_mers, 8, hipMemcpyDeviceToHost));
  const DevBloom B = b->view();
  const size_t nby = b->g.nbytes;
  const size_t lds0 = (size_t)kBloomChunk * 6 + (size_t)2 * nby * 2048, lds1 = (size_t)kPBlock * 5 * 6 + nby * 512;      // (bloom_ingest)
  const size_t lds2 = (size_t)nb * kBloomRingBytes + kBloomRingBytes + nby * 512;
  const BloomP1RingDirect rd{B.data, b2};
  std::string name;
#define KT_PB(N) do { KT_TRY(launch_lds(p1_bloom_granule_kernel<N>, dim3(grid), dim3(kPBlock), lds0, b->stream, B, BP, b->g, (const uint8_t*)d_bases, lo, hi, cap, d_gcur, d_tot, d_out, b->d_mers)); \
                      name = "p1_bloom_granule_kernel<" #N ">"; } while(0)
#define KT_PB2(N) do { KT_TRY(launch_lds(p1_bloom_granule2_kernel<N>, dim3(grid), dim3(kPBlock), lds1, b->stream, B, BP, b->g, (const uint8_t*)d_bases, lo, hi, cap, d_gcur, d_tot, d_out, b->d_mers)); \
                       name = "p1_bloom_granule2_kernel<" #N ">"; } while(0)
#define KT_PBR(N, PER) do { KT_TRY(launch_lds(p1_bloom_ring_kernel<N, PER>, dim3(grid), dim3(kPBlock), lds2, b->stream, B, BP, b->g, rd, (const uint8_t*)d_bases, lo, hi, cap, d_gcur, d_tot, d_out, b->d_mers, d_strag, d_strag_n)); \
                            name = "p1_bloom_ring_kernel<" #N "," #PER ">"; } while(0)
  if(family == 0) { if(nbt == 8) KT_PB(8); else if(nbt == 6) KT_PB(6); else KT_PB(0); }
  else if(family == 1) { if(nbt == 8) KT_PB2(8); else if(nbt == 6) KT_PB2(6); else KT_PB2(0); }
  else if(per == 10) { if(nbt == 8) KT_PBR(8, 10); else if(nbt == 6) KT_PBR(6, 10); else KT_PBR(0, 10); }
  else { if(nbt == 8) KT_PBR(8, 5); else KT_PBR(0, 5); }
#undef KT_PBR
#undef KT_PB2
#undef KT_PB
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(b->stream));
  HIP_TRY(hipMemcpy(strag, d_strag, (size_t)grid * kStragPerBlock * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(strag_n, d_strag_n, (size_t)grid * 4, hipMemcpyDeviceToHost));
  if(run_stragglers) {
    hipLaunchKernelGGL((p1_stragglers_kernel<uint32_t, BloomP1RingDirect>), dim3(b->n_cu), dim3(256), 0, b->stream, rd, (unsigned long long*)nullptr, (const uint64_t*)d_strag,
                       (const uint32_t*)d_strag_n, grid, cap, d_gcur, d_tot, d_out);
    name += "+p1_stragglers_kernel<uint32_t,BloomP1RingDirect>";
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(b->stream));
  }
  HIP_TRY(hipMemcpy(&m1, b->d_mers, 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out, d_out, ((size_t)nb + 1) * cap * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(gcur, d_gcur, 2 * (size_t)nb * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(tot, d_tot, (size_t)nb * 8, hipMemcpyDeviceToHost));
  if(mers) *mers = m1 - m0;
  say(launched, launched_len, name);
  return JFGPU_OK;
}

// ---- Tb alone ---------------------------------------------------------------------------------------------------------
// bloom_segment_kernel over segments [seg0, seg0 + n_seg) of the filter, `grid` workgroups; one to three item arrays: the items
// of segment seg0 + t in array s are items[off[t << sh] .. off[(t << sh) + 1]); sh = 1: all-ones entries are holes.
int jfkt_bloom_seg(jfgpu_bloom* b, uint32_t n_arr, const uint32_t* const* seg_items, const uint64_t* n_items, const uint64_t* const* seg_off,
                   const uint64_t* n_off, const uint32_t* sh, uint32_t n_seg, uint32_t seg0, uint32_t grid, char* launched, size_t launched_len) {
  int rc = kt_bloom_use(b, b ? b->bp : BloomPart{}, "jfkt_bloom_seg"); if(rc) return rc;
  if(!n_arr || n_arr > 3 || !n_seg || !grid || grid > 1024) return fail(JFGPU_E_INVALID, "jfkt_bloom_seg: one to three arrays, 1 <= grid <= 1024");
  if((uint64_t)seg0 + n_seg > b->bp.n_seg) return fail(JFGPU_E_INVALID, "jfkt_bloom_seg: segments beyond the filter");
  for(uint32_t s = 0; s < n_arr; ++s) {
    if(sh[s] > 1 || n_off[s] < (((uint64_t)n_seg - 1) << sh[s]) + 2) return fail(JFGPU_E_INVALID, "jfkt_bloom_seg: offsets do not cover the segments");
    for(uint32_t t = 0; t < n_seg; ++t) {
      const uint64_t a = seg_off[s][(size_t)t << sh[s]], e = seg_off[s][((size_t)t << sh[s]) + 1];
      if(a > e || e > n_items[s]) return fail(JFGPU_E_INVALID, "jfkt_bloom_seg: a segment's range lies outside the items");
      for(uint64_t i = a; i < e; ++i) {
        const uint32_t x = seg_items[s][i];
        if(!(sh[s] && x == 0xFFFFFFFFu) && (x & 7u) > 4u) return fail(JFGPU_E_INVALID, "jfkt_bloom_seg: an item's digit is five or more (a packed array holds no all-ones entry)");
      }
    }
  }
  DevBufs D;
  SegList S; memset(&S, 0, sizeof S);
  S.n = n_arr;
  for(uint32_t s = 0; s < n_arr; ++s) {
    uint32_t* di; uint64_t* doff;
    KT_TRY(D.put(&di, seg_items[s], (size_t)n_items[s], 4));
    KT_TRY(D.put(&doff, seg_off[s], (size_t)n_off[s]));
    S.items[s] = di; S.off[s] = doff; S.sh[s] = sh[s];
  }
  KT_TRY(launch_lds(bloom_segment_kernel, dim3(grid), dim3(kPBlock), (size_t)1 << kBloomSegBits, b->stream, b->view(), S, n_seg, seg0));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(b->stream));
  say(launched, launched_len, "bloom_segment_kernel");
  return JFGPU_OK;
}

// ---- the direct kernel of a small flush ----------------------------------------------------------------------------------
// bloom_items_direct_kernel over one granule batch: 2^b1 regions of cap entries, off[2 q], off[2 q + 1] the bounds of region q.
int jfkt_bloom_items_direct(jfgpu_bloom* b, uint32_t b1, uint32_t b2, uint32_t n_seg, const uint32_t* items, uint64_t n_items, const uint64_t* off, uint64_t n_off,
                            uint64_t cap, uint32_t grid, char* launched, size_t launched_len) {
  const BloomPart BP{b1, b2, n_seg, 0};
  int rc = kt_bloom_use(b, BP, "jfkt_bloom_items_direct"); if(rc) return rc;
  const uint64_t nb = 1ull << b1;
  if(!cap || n_items != nb * cap || n_off < 2 * nb || !grid || grid > 4096) return fail(JFGPU_E_INVALID, "jfkt_bloom_items_direct: a granule batch is 2^b1 regions of cap items");
  for(uint64_t q = 0; q < nb; ++q) {
    if(off[2 * q] != q * cap) return fail(JFGPU_E_INVALID, "jfkt_bloom_items_direct: a region starts at its own place");
    for(uint64_t v = q * cap; v < (q + 1) * cap && v < off[2 * q + 1]; ++v)
      if(items[v] != 0xFFFFFFFFu && !kt_bloom_item_ok(BP, (uint32_t)q, items[v])) return fail(JFGPU_E_INVALID, "jfkt_bloom_items_direct: an item names no cell of the filter");
  }
  DevBufs D;
  uint32_t* d_items; uint64_t* d_off;
  KT_TRY(D.put(&d_items, items, (size_t)n_items, 4));
  KT_TRY(D.put(&d_off, off, (size_t)n_off));
  hipLaunchKernelGGL(bloom_items_direct_kernel, dim3(grid), dim3(kBlock), 0, b->stream, b->view(), BP, (const uint32_t*)d_items, (const uint64_t*)d_off, cap);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(b->stream));
  say(launched, launched_len, "bloom_items_direct_kernel");
  return JFGPU_OK;
}

// ---- P2 with the Bloom functors ---------------------------------------------------------------------------------------------
// kernel 0: p2_granule_kernel<uint32_t, BloomDirect, kP2PairPer> on grid (4, nbk); 1: p2_ring_roles_kernel<uint32_t, 2,
// BloomRingDirect, 3> (nbk workgroups); 2: p2_ring_kernel<BloomRingDirect> on grid (4, nbk); 1 and 2 (b2 = 10 only, as on the
// host) are followed by p1_stragglers_kernel<uint32_t, BloomRingDirect>; all by granule_finish_range_kernel over the launched
// buckets' segments.  tag_bits = kBloomItemLow, arguments as bloom_flush_inner passes them.  Arrays as in jfkt_p2.
// out: 2^(b1 + b2) * cap2 items in and out; gcur: 2 * 2^(b1 + b2) words out; off2: 2 * 2^(b1 + b2) words in and out;
// ctr_direct: the functors' counter; strag_n: nbk (kernel 1) or 4 * nbk (kernel 2) list lengths.
int jfkt_bloom_p2(jfgpu_bloom* b, int kernel, uint32_t b1, uint32_t b2, uint32_t n_seg_f, uint32_t n_arr, const uint32_t* const* seg_items, const uint64_t* n_items,
                  const uint64_t* const* seg_off, const uint64_t* n_off, const uint32_t* sh, uint32_t cap2, uint32_t bucket0, uint32_t nbk,
                  uint32_t* out, uint32_t* gcur, uint64_t* off2, uint64_t* ctr_direct, uint32_t* strag_n, char* launched, size_t launched_len) {
  const BloomPart BP{b1, b2, n_seg_f, 0};
  int rc = kt_bloom_use(b, BP, "jfkt_bloom_p2"); if(rc) return rc;
  if(kernel < 0 || kernel > 2 || !n_arr || n_arr > (uint32_t)kMaxSeg || !nbk || !cap2 || cap2 % kGran) return fail(JFGPU_E_INVALID, "jfkt_bloom_p2: bad kernel, array count, bucket count or capacity");
  if(b2 > 10 || (kernel != 0 && b2 != 10)) return fail(JFGPU_E_INVALID, "jfkt_bloom_p2: at most 1024 segments a bucket; the ring kernels take exactly 1024");
  if((uint64_t)bucket0 + nbk > (1ull << b1)) return fail(JFGPU_E_INVALID, "jfkt_bloom_p2: launched buckets beyond 2^b1");
  if(kernel != 0 && (((uint64_t)bucket0 + nbk) << b2) > n_seg_f) return fail(JFGPU_E_INVALID, "jfkt_bloom_p2: the ring kernels take buckets whose segments all exist");
  for(uint32_t s = 0; s < n_arr; ++s) {
    const uint64_t need = ((uint64_t)(bucket0 + nbk - 1) << sh[s]) + 2;
    if(sh[s] > 1 || n_off[s] < need) return fail(JFGPU_E_INVALID, "jfkt_bloom_p2: offsets do not cover the launched buckets");
    if(kernel == 2 && sh[s] != 1) return fail(JFGPU_E_INVALID, "jfkt_bloom_p2: the shared-ring kernel takes granule arrays only");
    for(uint32_t j = bucket0; j < bucket0 + nbk; ++j) {
      const uint64_t a = seg_off[s][(size_t)j << sh[s]], e = seg_off[s][((size_t)j << sh[s]) + 1];
      if(a > e || e > n_items[s]) return fail(JFGPU_E_INVALID, "jfkt_bloom_p2: a bucket's range lies outside its array");
      if(kernel != 0 && sh[s] == 1 && (a % 4)) return fail(JFGPU_E_INVALID, "jfkt_bloom_p2: a granule region starts at a multiple of 16 bytes");
      for(uint64_t i = a; i < e; ++i) {
        const uint32_t x = seg_items[s][i];
        if(!(sh[s] && x == 0xFFFFFFFFu) && !kt_bloom_item_ok(BP, j, x)) return fail(JFGPU_E_INVALID, "jfkt_bloom_p2: an item names no cell of the filter");
      }
    }
  }
  const size_t n_dest = (size_t)1 << (b1 + b2);
  DevBufs D;
  SegList S; memset(&S, 0, sizeof S);
  S.n = n_arr;
  for(uint32_t s = 0; s < n_arr; ++s) {
    uint32_t* di; uint64_t* doff;
    KT_TRY(D.put(&di, seg_items[s], (size_t)n_items[s], 4));
    KT_TRY(D.put(&doff, seg_off[s], (size_t)n_off[s]));
    S.items[s] = di; S.off[s] = doff; S.sh[s] = sh[s];
  }
  const uint32_t n_lists = kernel == 1 ? nbk : kG2Blocks * nbk;
  uint32_t *d_out, *d_strag_n; unsigned int* d_gcur; uint64_t *d_strag, *d_off2; unsigned long long* d_ctr;
  KT_TRY(D.put(&d_out, out, n_dest * cap2));
  KT_TRY(D.get(&d_gcur, 2 * n_dest, 0));
  KT_TRY(D.put(&d_off2, off2, 2 * n_dest));
  KT_TRY(D.get(&d_strag, (size_t)n_lists * kP2StragPerBlock, 0));
  KT_TRY(D.get(&d_strag_n, n_lists, 0));
  KT_TRY(D.get(&d_ctr, 1, 0));
  const DevBloom B = b->view();
  const BloomDirect DD{B, BP, d_ctr};
  const BloomRingDirect RD{B.data};
  const dim3 block(kPBlock);
  const size_t rl = ((size_t)1 << b2) * 128 + 128;
  std::string name;
  if(kernel == 0) {
    KT_TRY(launch_lds(p2_granule_kernel<uint32_t, BloomDirect, kP2PairPer>, dim3(kG2Blocks, nbk), block, (size_t)kPBlock * kP2PairPer * sizeof(uint32_t), b->stream,
                       DD, b2, kBloomItemLow, S, cap2, d_gcur, d_gcur + n_dest, d_out, bucket0, (unsigned long long*)nullptr, 0xFFFFFFFFu));
    name = "p2_granule_kernel<uint32_t,BloomDirect,kP2PairPer>";
  } else {
    if(kernel == 1) {
      KT_TRY(launch_lds(p2_ring_roles_kernel<uint32_t, 2, BloomRingDirect, 3>, dim3(nbk), block, rl, b->stream, RD, b2, kBloomItemLow, S, cap2, d_gcur,
                         d_out, bucket0, d_strag, d_strag_n, d_ctr));
      name = "p2_ring_roles_kernel<uint32_t,2,BloomRingDirect,3>";
    } else {
      KT_TRY(launch_lds(p2_ring_kernel<BloomRingDirect>, dim3(kG2Blocks, nbk), block, rl, b->stream, RD, b2, kBloomItemLow, S, cap2, d_gcur, d_gcur + n_dest,
                         d_out, bucket0, (unsigned long long*)nullptr, d_strag, d_strag_n, d_ctr));
      name = "p2_ring_kernel<BloomRingDirect>";
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((p1_stragglers_kernel<uint32_t, BloomRingDirect>), dim3(b->n_cu), dim3(256), 0, b->stream, RD, d_ctr, (const uint64_t*)d_strag, (const uint32_t*)d_strag_n,
                       n_lists, cap2, d_gcur, (unsigned long long*)nullptr, d_out, kP2StragPerBlock);
    name += "+p1_stragglers_kernel<uint32_t,BloomRingDirect>";
  }
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(granule_finish_range_kernel, dim3(256), dim3(256), 0, b->stream, d_gcur, cap2, (uint32_t)n_dest, d_off2, bucket0 << b2, nbk << b2);
  name += "+granule_finish_range_kernel";
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(b->stream));
  HIP_TRY(hipMemcpy(out, d_out, n_dest * cap2 * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(gcur, d_gcur, 2 * n_dest * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(off2, d_off2, 2 * n_dest * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ctr_direct, d_ctr, 8, hipMemcpyDeviceToHost));
  if(strag_n) HIP_TRY(hipMemcpy(strag_n, d_strag_n, (size_t)n_lists * 4, hipMemcpyDeviceToHost));
  say(launched, launched_len, name);
  return JFGPU_OK;
}

}  // extern "C"
