// jellyfish_amd/csrc/kernels_nword_part.hip.hpp -- the partitioned insert path for keys of three and four words
// (65 <= k <= 128), gfx950.  The three stages of kernels_part.hip.hpp and kernels_wide_part.hip.hpp -- no global atomic
// on the hot path:
//
//   P1n  p1_nword_granule_kernel: encode + canonical + GF(2) hash of 256-bit k-mers (staged and walked as
//        KeyOps<NTable>::stage_tile / for_each_kmer_nword do), 256-bit items counting-sorted by the upper tile bits in LDS
//        and written as whole runs into fixed bucket regions (granule_emit)
//   P2   the exact scheme of kernels_part.hip.hpp -- p2_kernel / scan_matrix_kernel / p2_scatter_sorted_kernel -- with
//        ITEM = u256, a value type with exactly the operators those templates use
//   Tn   tile_insert_nword_kernel: one workgroup owns one tile of 2048 x 32 B = 64 KiB in LDS; the four-word claim of
//        kernels_nword.hip.hpp (CAS hi 0 -> occ|tag_hi, then CAS lo_i 0 -> lo_i, add to hi) on LDS words
//
// item = (tile_rest << tag_full) | tag,  tag = (idx0 << rem_bits) | (key >> lsize): make_item_wide with K256 arithmetic,
// 2k - b1 bits in all, in 32 bytes.  All ones is the hole, as for the other item widths; an item is never all ones because
// it never has 256 bits (host_partition.inl: part_geom_init refuses a geometry whose items would).
// The table format is the one of kernels_nword.hip.hpp, so look-ups, stats, growth, the sorted dump and the shard code do
// not care which path inserted a key.
//
// LDS: P1n 32 KiB of items + 2 KiB of bucket ids + the forward byte tables of the hash (ceil(2k / 8) x 2 KiB: 50 KiB at
// k = 100, 64 KiB at k = 128), all dynamic, + GranuleLds 34 KiB + the staged codes 8 KiB = 126 - 140 KiB, one workgroup of
// 1024 a CU;  P2 scatter 3 items a lane = 96 KiB + 24 KiB of cursors;  Tn 64 KiB, two workgroups of 512 a CU.
// (The tables were first read through the caches, in rounds of 2048 items: 154 ms of P1 for 680 M 100-mers, as slow as the
// direct kernel's 236 ms of hash + claims (107 - 111 ms from LDS) -- 50 KiB of table do not stay in a CU's 32 KiB of L1, so nearly every one of a
// k-mer's 25 gathers fetched a line from L2.  profiles/nword_part_rate.txt has both.)
#pragma once
#include "kernels_part.hip.hpp"
#include "kernels_nword.hip.hpp"

namespace jfgpu {

// A 256-bit item: what the ITEM templates of kernels_part.hip.hpp ask of their type -- construction from an integer, ~, ==,
// >>, & and narrowing to 64 and 32 bits.  Loaded and stored as two 16-byte accesses.
struct alignas(16) u256 {
  K256 v;
  u256() = default;
  JF_HD u256(uint64_t x) : v(k256_from64(x)) {}
  JF_HD u256(int x) : v(k256_from64((uint64_t)x)) {}
  JF_HD explicit u256(const K256& k) : v(k) {}
  JF_HD u256 operator~() const { u256 r; for(int i = 0; i < 4; ++i) r.v.w[i] = ~v.w[i]; return r; }
  JF_HD bool operator==(const u256& o) const { return k256_eq(v, o.v); }
  JF_HD u256 operator>>(uint32_t n) const { return u256(k256_shr(v, n)); }
  JF_HD u256 operator&(const u256& o) const { return u256(k256_and(v, o.v)); }
  JF_HD explicit operator uint64_t() const { return v.w[0]; }
  JF_HD explicit operator uint32_t() const { return (uint32_t)v.w[0]; }
};
static_assert(sizeof(u256) == 32, "a 256-bit item is 32 bytes");

constexpr int kNPer = 1;                                     // items per lane per round of the P1 kernel
constexpr int kNChunk = kPBlock * kNPer;                     // 1024 items = 32 KiB of LDS
JF_HD constexpr size_t p1_nword_lds(uint32_t nbytes) { return (size_t)kNChunk * 34 + (size_t)nbytes * 2048; }    // items, bucket ids, byte tables
constexpr int kNTileBlock = 512;                             // threads of a Tn workgroup: two workgroups (64 KiB each) a CU
constexpr int kP2NWordPer = 3;                               // items per lane and chunk of the P2 scatter: 3 Ki items = 96 KiB

__device__ inline u256 make_item_nword(const NGeom& N, const PartGeom& P, const K256& key, uint64_t local) {
  const uint64_t rest = local & ((1ull << P.rest_shift) - 1);            // tile_rest (b2 bits) above idx0 (tile_bits)
  return u256(k256_or(k256_shl(k256_from64(rest), N.g.rem_bits), k256_shr(key, N.g.lsize_g)));
}

// what an item says of its slot: the tile-local start of the probe sequence and the slot words
struct NItemSlot { uint32_t idx0; NSlot w; };
__device__ inline NItemSlot nword_item_slot(const NGeom& N, const u256& it) {
  const K256 tag = k256_and(it.v, k256_low_mask(N.tag_full));
  NItemSlot s;
  s.idx0 = (uint32_t)k256_shr(tag, N.g.rem_bits).w[0];
  s.w = nword_tag_words(N, tag);
  return s;
}

// One item of P1 bucket `bucket` straight into the table: the global claim of nword_add_at.
template <bool RETURNING>
__device__ inline void nword_item_direct(const NTable& T, const PartGeom& P, uint32_t bucket, const u256& it) {
  const uint64_t tile = ((uint64_t)bucket << P.b2) | (k256_shr(it.v, T.N.tag_full).w[0] & ((1ull << P.b2) - 1));
  const NItemSlot s = nword_item_slot(T.N, it);
  nword_claim<RETURNING>(T, s.w, tile << T.N.g.tile_bits, s.idx0, 1);
}

// what to do with an item its region cannot take (the counterpart of WideDirect)
template <bool RETURNING>
struct NWordDirect {
  NTable T; PartGeom P;
  __device__ void operator()(uint32_t bucket, const u256& item) const { nword_item_direct<RETURNING>(T, P, bucket, item); }
  __device__ unsigned long long* direct_counter() const { return (unsigned long long*)&T.counters[CTR_DIRECT]; }
};

// hash_tables_n256 on byte tables staged in LDS: the key's words taken one at a time (no indexing of the key by a run-time
// byte number, which would put it in scratch), the byte count a wave-uniform bound
__device__ inline uint64_t hash_lds_n256(const uint64_t* s_tbl, const K256& key, uint32_t nbytes) {
  uint64_t pos = 0;
#pragma unroll
  for(uint32_t q = 0; q < 4; ++q) {
    const uint64_t w = key.w[q];
#pragma unroll
    for(uint32_t i = 0; i < 8; ++i) {
      const uint32_t b = 8 * q + i;
      if(b < nbytes) pos ^= s_tbl[b * 256 + ((w >> (8 * i)) & 0xFF)];
    }
  }
  return pos;
}

// ---- P1n --------------------------------------------------------------------------------------------------
// One block iteration = 16384 sequence positions, in rounds of kNPer positions per lane (1024 items per round).  The walk is
// for_each_kmer_nword's, a round at a time: the roll of the forward and the reverse-complement key, the validity window
// (`filled`), the canonical choice by k256_less.
template <bool RETURNING>
__global__ __launch_bounds__(kPBlock) void p1_nword_granule_kernel(NTable T, PartGeom P, const uint8_t* __restrict__ base, int64_t lo, int64_t hi,
                                                                   uint32_t cap, unsigned int* __restrict__ gcur,
                                                                   unsigned long long* __restrict__ tot, u256* __restrict__ out) {
  JF_DYN_LDS(s_dyn);
  u256* s_item = reinterpret_cast<u256*>(s_dyn);                                       // [kNChunk]
  uint16_t* s_bkt = reinterpret_cast<uint16_t*>(s_dyn + (size_t)kNChunk * 32);         // [kNChunk]
  uint64_t* s_fwd = reinterpret_cast<uint64_t*>(s_dyn + (size_t)kNChunk * 34);         // [nbytes * 256]
  __shared__ uint32_t s_codes[kPBlock + 8];
  __shared__ uint32_t s_inv[kPBlock + 8];
  __shared__ GranuleLds G;
  const NGeom& N = T.N;
  const TableGeom& g = N.g;
  const uint32_t nb = 1u << P.b1;
  load_tables_lds(s_fwd, T.fwd_tbl, g.nbytes);
  granule_init(G, nb);
  const uint32_t k = g.k, rc_pos = 2 * (k - 1), bshift = g.lsize_l - P.b1;
  uint32_t my_mers = 0, my_direct = 0;
  const int64_t n_tiles = (hi + kPTilePos - 1) / kPTilePos;
  for(int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    __syncthreads();
    NLane L = KeyOps<NTable>::stage_tile(T, base, tile * kPTilePos, lo, hi, s_codes, s_inv);   // barrier inside
#pragma unroll 1
    for(int j0 = 0; j0 < kPerLane; j0 += kNPer) {
      lds_barrier();
      for(uint32_t q = threadIdx.x; q < nb; q += blockDim.x) G.hist[q] = 0;
      lds_barrier();
      u256 it[kNPer]; uint32_t dr[kNPer];
#pragma unroll
      for(int e = 0; e < kNPer; ++e) {
        const int j = j0 + e;
        dr[e] = 0xFFFFFFFFu; it[e] = 0;
        const uint64_t code = (L.c >> (2 * (15 - j))) & 3u;
        k256_roll_fw(L.fw, code, N.key_mask);
        k256_roll_rc(L.rc, 3ull - code, rc_pos);
        if((L.v >> (15 - j)) & 1u) { L.filled = 0; continue; }
        if(L.filled < k) ++L.filled;
        if(L.filled < k) continue;
        ++my_mers;
        const K256 key = (g.canonical && k256_less(L.rc, L.fw)) ? L.rc : L.fw;
        const uint64_t local = hash_lds_n256(s_fwd, key, g.nbytes) & g.local_mask;
        const uint32_t b = P.b1 ? (uint32_t)(local >> bshift) : 0u;
        it[e] = make_item_nword(N, P, key, local);
        dr[e] = (b << 16) | atomicAdd(&G.hist[b], 1u);
      }
      my_direct += granule_emit(G, nb, cap, gcur, out, s_item, s_bkt, it, dr,
                                [&](uint32_t b, const u256& v) { nword_item_direct<RETURNING>(T, P, b, v); });
    }
  }
  granule_finish(G, nb, cap, tot, out);
  if(my_direct) atomicAdd((unsigned long long*)&T.counters[CTR_DIRECT], (unsigned long long)my_direct);
  uint64_t w = my_mers;
  for(int o = 32; o > 0; o >>= 1) w += __shfl_down(w, o, 64);
  if((threadIdx.x & 63) == 0 && w) atomicAdd((unsigned long long*)&T.counters[CTR_MERS], (unsigned long long)w);
}

// ---- Tn: one workgroup owns one 64 KiB tile in LDS ------------------------------------------------------------
// The claim order is nword_claim's: hi, then lo0, lo1, lo2; a lane goes on only while every word so far is its own.
template <bool RETURNING>
__device__ inline void tile_insert_nword_one(const NTable& T, unsigned long long* s_tile, const u256& item, uint64_t tile_index) {
  const TableGeom& g = T.N.g;
  const NItemSlot s = nword_item_slot(T.N, item);
  const uint32_t tmask = (uint32_t)g.tile_mask;
  for(uint32_t p = 0; p <= T.max_probe; ++p) {
    const uint32_t slot = probe_slot(s.idx0, p, tmask);
    unsigned long long* sp = &s_tile[4 * slot];
    const unsigned long long old = atomicCAS(sp + 3, 0ull, (unsigned long long)s.w.hi_low);
    if(old != 0ull && (old & g.low_mask) != s.w.hi_low) continue;
    bool mine = true;
    for(uint32_t i = 0; i < 3 && mine; ++i) {
      const unsigned long long l = atomicCAS(sp + i, 0ull, (unsigned long long)s.w.lo[i]);
      if(l != 0ull && l != s.w.lo[i]) mine = false;
    }
    if(!mine) continue;
    if(RETURNING) {      // count fields under 40 bits (k >= 107): what passes cnt_max goes to the overflow table, as nword_add_at<true>
      const unsigned long long prev = atomicAdd(sp + 3, (unsigned long long)g.inc);
      if((prev >> (g.tag_bits + 1)) + 1 > g.cnt_max) { const DevTable d = ovf_view(T); ovf_add(d, (tile_index << g.tile_bits) + slot, 1); }
    } else {
      atomicAdd(sp + 3, (unsigned long long)g.inc);
    }
    return;
  }
  atomicAdd((unsigned long long*)&T.counters[CTR_FULL], 1ull);
}

// The tile is always loaded: NTable carries no dirty bytes (the direct kernel of these keys never set them), and a load of
// an all-zero tile costs what zeroing it in LDS and storing it costs anyway.
template <bool RETURNING>
__global__ __launch_bounds__(kNTileBlock) void tile_insert_nword_kernel(NTable T, SegList S, uint64_t tile0, uint32_t n_tiles) {
  JF_DYN_LDS(s_raw);
  unsigned long long* s_tile = reinterpret_cast<unsigned long long*>(s_raw);
  const TableGeom& g = T.N.g;
  const uint32_t words = (uint32_t)kNWords << g.tile_bits;             // 64-bit words of one tile
  for(uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    uint64_t n_items = 0;
    for(uint32_t s = 0; s < S.n; ++s) n_items += seg_hi(S, s, t) - seg_lo(S, s, t);
    if(n_items == 0) continue;                                          // block-uniform
    uint64_t* gt = T.slots + ((tile0 + t) << (g.tile_bits + 2));
    for(uint32_t i = threadIdx.x * 2; i < words; i += blockDim.x * 2)
      *reinterpret_cast<ulonglong2*>(s_tile + i) = *reinterpret_cast<const ulonglong2*>(gt + i);
    lds_barrier();
    for(uint32_t s = 0; s < S.n; ++s) {
      const uint64_t a = seg_lo(S, s, t), b = seg_hi(S, s, t);
      const u256* src = reinterpret_cast<const u256*>(S.items[s]);
      const bool holes = S.sh[s] != 0;
      const u256 hole = ~u256(0);
      constexpr int U = 2;                                              // 32-byte loads in flight per lane
      for(uint64_t v0 = a + threadIdx.x; v0 < b; v0 += (uint64_t)U * blockDim.x) {
        u256 x[U];
#pragma unroll
        for(int u = 0; u < U; ++u) { const uint64_t v = v0 + (uint64_t)u * blockDim.x; x[u] = v < b ? src[v] : hole; }
#pragma unroll
        for(int u = 0; u < U; ++u) {
          const uint64_t v = v0 + (uint64_t)u * blockDim.x;
          if(v < b && !(holes && x[u] == hole)) tile_insert_nword_one<RETURNING>(T, s_tile, x[u], tile0 + t);
        }
      }
    }
    lds_barrier();
    for(uint32_t i = threadIdx.x * 2; i < words; i += blockDim.x * 2)
      *reinterpret_cast<ulonglong2*>(gt + i) = *reinterpret_cast<const ulonglong2*>(s_tile + i);
    lds_barrier();
  }
}

// Too few items to be worth streaming the tiles: pending granule batches inserted with global atomics.
template <bool RETURNING>
__global__ __launch_bounds__(kBlock) void items_direct_nword_kernel(NTable T, PartGeom P, const u256* __restrict__ items,
                                                                    const uint64_t* __restrict__ off, uint64_t cap) {
  const uint32_t nb = 1u << P.b1;
  const uint64_t n = (uint64_t)nb * cap;
  const u256 hole = ~u256(0);
  for(uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t b = (uint32_t)(v / cap);
    if(v >= off[2 * (size_t)b + 1]) continue;
    const u256 it = items[v];
    if(it == hole) continue;
    nword_item_direct<RETURNING>(T, P, b, it);
  }
}

}  // namespace jfgpu
