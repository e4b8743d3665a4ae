// jellyfish_amd/csrc/kernels_bloom_part_keys.hip.hpp -- P1b of the partitioned Bloom insert for keys of two, three and four
// words (33 <= k <= 128), gfx950.  Included by kernels_bloom_part.hip.hpp.
//
// From P2 onwards a Bloom item is a 32-bit cell update that says nothing of the key's width, so the wider keys need a P1b
// of their own and nothing else: p1_bloom_keys_kernel<Table, PER> stages and walks a tile as KeyOps<Table> does over
// geom_view(G) (the way bloom_query_ascii_kernel obtains its view, the walk of p1_nword_granule_kernel: one position a
// round, block-uniform, roll + validity window + canonical choice inside the round), takes both 64-row products from
// nibble tables in LDS and hands cell and increment to bloom_p1_emit_cells, the rounds of the one-word kernels.
//
// LDS: kPBlock * PER * 6 bytes of sort buffers + B.nbytes * 512 of nibble tables (16 entries of one uint4 -- both hashes --
// per key nibble: 8 KiB at k = 64, 16 KiB at k = 128; byte tables would take 128 KiB), dynamic; GranuleLds 34 KiB and the
// staged codes 8 KiB, static.  PER = 10: 118 KiB at k = 128, one workgroup of 1024 a CU, so a lane may hold 128 vector
// registers -- the forward and reverse-complement keys of a four-word view are 16 of them before anything else, and
// neither instantiation fits the 64 that two workgroups a CU would leave (profiles/bloom_keys_p1_resources.txt).
#pragma once
#include "kernels_wide.hip.hpp"
#include "kernels_nword.hip.hpp"
#include "kernels_bloom_query.hip.hpp"

namespace jfgpu {

constexpr int kBloomKeysPer = 10;                            // cell updates per lane and round
JF_HD constexpr size_t p1_bloom_keys_lds(uint32_t nbytes, int per = kBloomKeysPer) { return (size_t)kPBlock * per * 6 + (size_t)nbytes * 512; }

// What P1b asks of a key view beyond KeyOps: the geometry the kernel is handed, and the walk of a staged lane one position
// at a time.  step(): roll position j in; true when a k-mer ends there, its (canonical) key in w[], lowest word first.
template <class Table> struct BloomKeyWalk;

template <> struct BloomKeyWalk<WideTable> {
  typedef WideGeom Geom;
  static constexpr int kWords = 2;
  struct State { u128 fw, rc; };
  __device__ static State begin(const WideTable& T, const LaneWordsW& L) {
    State S;
    S.fw = ((((u128)L.p4 << 96) | ((u128)L.p3 << 64) | ((u128)L.p2 << 32) | L.p1)) & T.W.key_mask;
    S.rc = revcomp128(S.fw, T.W.g.k);
    return S;
  }
  __device__ static bool step(const WideTable& T, const LaneWordsW& L, State& S, int j, uint64_t (&w)[kWords]) {
    const uint32_t k = T.W.g.k;
    const uint64_t c = (L.cur >> (2 * (15 - j))) & 3u;
    S.fw = ((S.fw << 2) | c) & T.W.key_mask;
    S.rc = (S.rc >> 2) | ((u128)(3ull - c) << (2 * (k - 1)));
    const u128 kwin = (((u128)1) << k) - 1;                 // k <= 64
    if(((L.inv80 >> (15 - j)) & kwin) != 0) return false;
    const u128 key = (T.W.g.canonical && S.rc < S.fw) ? S.rc : S.fw;
    w[0] = (uint64_t)key; w[1] = (uint64_t)(key >> 64);
    return true;
  }
};

// k256_shr and k256_roll_rc (kernels_nword.hip.hpp) index a key's words by a run-time number, which puts the key in scratch
// (88 bytes a lane in every kernel that calls them).  The same two steps with every word index a constant: selects instead.
__device__ __forceinline__ K256 k256_shr_reg(const K256& a, uint32_t n) {          // n < 256
  const uint32_t ws = n >> 6, bs = n & 63;
  K256 r;
#pragma unroll
  for(uint32_t i = 0; i < 4; ++i) {
    uint64_t lo = 0, hi = 0;
#pragma unroll
    for(uint32_t s = 0; s < 4; ++s)
      if(ws == s) { lo = i + s < 4 ? a.w[i + s < 4 ? i + s : 0] : 0; hi = i + s + 1 < 4 ? a.w[i + s + 1 < 4 ? i + s + 1 : 0] : 0; }
    r.w[i] = bs ? (lo >> bs) | (hi << (64 - bs)) : lo;
  }
  return r;
}
__device__ __forceinline__ K256 revcomp256_reg(const K256& x, uint32_t k) {
  K256 r;
#pragma unroll
  for(int i = 0; i < 4; ++i) r.w[i] = revcomp64(x.w[3 - i], 32);
  return k256_shr_reg(r, 256 - 2 * k);
}
__device__ __forceinline__ void k256_roll_rc_reg(K256& x, uint64_t v, uint32_t bitpos) {
  x.w[0] = (x.w[0] >> 2) | (x.w[1] << 62);
  x.w[1] = (x.w[1] >> 2) | (x.w[2] << 62);
  x.w[2] = (x.w[2] >> 2) | (x.w[3] << 62);
  x.w[3] = x.w[3] >> 2;
  const uint32_t at = bitpos >> 6;
  const uint64_t bits = v << (bitpos & 63);
#pragma unroll
  for(uint32_t q = 0; q < 4; ++q) x.w[q] |= at == q ? bits : 0ull;
}

template <> struct BloomKeyWalk<NTable> {
  typedef NGeom Geom;
  static constexpr int kWords = 4;
  typedef NLane State;
  // (the staged lane's own reverse complement is not read: computed here with constant word indices, the staging's is dead code)
  __device__ static State begin(const NTable& T, const NLane& L) { State S = L; S.rc = revcomp256_reg(L.fw, T.N.g.k); return S; }
  __device__ static bool step(const NTable& T, const NLane&, State& S, int j, uint64_t (&w)[kWords]) {
    const uint32_t k = T.N.g.k;
    const uint64_t code = (S.c >> (2 * (15 - j))) & 3u;
    k256_roll_fw(S.fw, code, T.N.key_mask);
    k256_roll_rc_reg(S.rc, 3ull - code, 2 * (k - 1));
    if((S.v >> (15 - j)) & 1u) { S.filled = 0; return false; }
    if(S.filled < k) ++S.filled;
    if(S.filled < k) return false;
    // (by mask: `r ? S.rc : S.fw` becomes a choice between two addresses, and the state goes to scratch to have some)
    const uint64_t r = (T.N.g.canonical && k256_less(S.rc, S.fw)) ? ~0ull : 0ull;
#pragma unroll
    for(int q = 0; q < kWords; ++q) w[q] = (S.rc.w[q] & r) | (S.fw.w[q] & ~r);
    return true;
  }
};

// Both 64-row products of a key of KW words from the nibble tables: entry (nibble n, value v) at s_tn[16 n + v] holds
// (h0 low, h0 high, h1 low, h1 high).  Exactly 2 * nbytes nibbles are read: four key bytes the key fills take their eight
// gathers with no test between them, the last, partial four one wave-uniform test a byte.  The key's words are taken one at a time
// (no indexing by a run-time byte number, which would put the key in scratch).
template <int KW>
__device__ __forceinline__ void bloom_hash2_nibbles(const uint4* s_tn, const uint64_t (&w)[KW], uint32_t nbytes, uint64_t& h0, uint64_t& h1) {
  uint32_t a0 = 0, a1 = 0, c0 = 0, c1 = 0;
  auto byte = [&](uint64_t word, uint32_t q, uint32_t i) {
    const uint32_t n = 16 * q + 2 * i;
    const uint4 e = s_tn[n * 16 + ((uint32_t)(word >> (8 * i)) & 15u)], f = s_tn[(n + 1) * 16 + ((uint32_t)(word >> (8 * i + 4)) & 15u)];
    a0 ^= e.x ^ f.x; a1 ^= e.y ^ f.y; c0 ^= e.z ^ f.z; c1 ^= e.w ^ f.w;
  };
#pragma unroll
  for(uint32_t q = 0; q < (uint32_t)KW; ++q) {
    const uint64_t word = w[q];
#pragma unroll
    for(uint32_t h = 0; h < 8; h += 4) {                     // four key bytes a test: eight gathers (32 registers) in flight
      if(nbytes >= 8 * q + h + 4) {
#pragma unroll
        for(uint32_t i = h; i < h + 4; ++i) byte(word, q, i);
      } else {
#pragma unroll
        for(uint32_t i = h; i < h + 4; ++i) if(8 * q + i < nbytes) byte(word, q, i);
      }
    }
  }
  h0 = ((uint64_t)a1 << 32) | a0; h1 = ((uint64_t)c1 << 32) | c0;
}

template <class Table, int PER>
__global__ __launch_bounds__(kPBlock) void p1_bloom_keys_kernel(DevBloom B, BloomPart BP, typename BloomKeyWalk<Table>::Geom Gm, const uint8_t* __restrict__ base,
                                                                int64_t lo, int64_t hi, uint32_t cap,
                                                                unsigned int* __restrict__ gcur, unsigned long long* __restrict__ tot,
                                                                uint32_t* __restrict__ out, unsigned long long* __restrict__ mers) {
  typedef KeyOps<Table> K;
  typedef BloomKeyWalk<Table> W;
  constexpr int kChunk = kPBlock * PER;
  JF_DYN_LDS(s_dyn);
  uint32_t* s_item = reinterpret_cast<uint32_t*>(s_dyn);                               // [kChunk]
  uint16_t* s_bkt = reinterpret_cast<uint16_t*>(s_dyn + (size_t)kChunk * 4);           // [kChunk]
  uint4* s_tn = reinterpret_cast<uint4*>(s_dyn + (size_t)kChunk * 6);                  // [nbytes * 32]
  __shared__ uint32_t s_codes[kPBlock + K::kHaloWords];
  __shared__ uint32_t s_inv[kPBlock + K::kHaloWords];
  __shared__ GranuleLds G;
  const Table T = geom_view(Gm);
  const uint32_t nb = 1u << BP.b1;
  bloom_nibble_tables_lds(s_tn, B);
  granule_init(G, nb);
  uint32_t my_mers = 0, my_direct = 0;
  const int64_t n_tiles = (hi + kPTilePos - 1) / kPTilePos;
  for(int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    __syncthreads();
    const typename K::Lane L = K::stage_tile(T, base, tile * kPTilePos, lo, hi, s_codes, s_inv);     // barrier inside
    typename W::State S = W::begin(T, L);
#pragma unroll 1
    for(int j = 0; j < kPerLane; ++j) {
      uint64_t key[W::kWords];
      const bool valid = W::step(T, L, S, j, key);
      uint64_t cell = 0, inc = 0;
      if(valid) {
        ++my_mers;
        uint64_t h0, h1;
        bloom_hash2_nibbles<W::kWords>(s_tn, key, B.nbytes, h0, h1);
        cell = bloom_mod(h0, B.m, B.recip);
        inc = bloom_mod(h1, B.m, B.recip);
      }
      // (every lane reaches the rounds, with or without a k-mer: granule_emit has barriers)
      my_direct += bloom_p1_emit_cells<PER>(B, BP, G, nb, cap, gcur, out, s_item, s_bkt, valid, cell, inc);
    }
  }
  granule_finish(G, nb, cap, tot, out);
  bloom_p1_add_mers(mers, my_mers);
  (void)my_direct;
}

}  // namespace jfgpu
