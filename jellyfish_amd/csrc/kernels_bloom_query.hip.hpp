// jellyfish_amd/csrc/kernels_bloom_query.hip.hpp -- query: check() of every k-mer of a contract buffer against a Bloom counter.
//
// Reference (paths relative to the reference's source tree):
//   sub_commands/query_main.cc:44-51   query_from_sequence: mer_iterator over the sequence, db.check(*mers) per k-mer
//   sub_commands/query_main.cc:99-104  the database is a mer_dna_bloom_counter when the header says "bloomcounter"
//   include/jellyfish/bloom_counter2.hpp:109-142  check__: the minimum of the k-mer's nb_hashes cells, 0, 1 or 2
// One kernel for the three key views (one, two, three and four words): the tile loop of the bloom_insert_ascii kernels
// with bloom_check where they insert, and the output convention of query_ascii_kernel (kernels.hip.hpp) -- vals[p] and
// flags[p] indexed by the position of the window's last base, every entry of [0, hi - lo) written, nothing else.  What a
// view contributes comes from its KeyOps (staging, rolling, text_key, same_key); the table those take is a view that holds
// the counter's geometry and nothing else (geom_view).  The counter is only read: no atomics, the k-mer tally untouched.
// A lane's 16 answers are two bits each and its flags two bit masks (three registers, no arrays) until they are stored.
// LDS, all static: the tile's codes and invalid masks, and for one-word keys the two matrices' byte tables (32 KiB, as
// bloom_insert_ascii_kernel); the wider views read theirs through the caches like their insert kernels.
#pragma once
#include <type_traits>

namespace jfgpu {

// bloom_check with the cell reads of a k-mer issued four at a time before any of them is used: they do not depend on
// each other (cell i is base + i * inc mod m), and one at a time a lane pays nh dependent round trips to HBM.
__device__ inline uint32_t bloom_check_ahead(const DevBloom& B, uint64_t h0, uint64_t h1) {
  constexpr uint32_t kAhead = 4;
  const uint64_t inc = bloom_mod(h1, B.m, B.recip);
  uint64_t p = bloom_mod(h0, B.m, B.recip);
  uint32_t res = 2;
  for(uint32_t i = 0; i < B.nh; i += kAhead) {
    uint64_t byte[kAhead]; uint32_t dig[kAhead], w[kAhead];
#pragma unroll
    for(uint32_t e = 0; e < kAhead; ++e) {
      divmod5(p, byte[e], dig[e]);
      w[e] = i + e < B.nh ? B.data[byte[e] >> 2] : 0u;
      p += inc; if(p >= B.m) p -= B.m;
    }
#pragma unroll
    for(uint32_t e = 0; e < kAhead; ++e) {
      const uint32_t d = i + e < B.nh ? bloom_digit((w[e] >> (8 * (uint32_t)(byte[e] & 3))) & 0xFFu, dig[e]) : 2u;
      res = d < res ? d : res;
    }
  }
  return res;
}

// a key's product with one of the counter's matrices, by the byte tables of the key's width
__device__ inline uint64_t bloom_hash(const uint64_t* tbl, uint64_t key, uint32_t nbytes) { return hash_tables(tbl, key, nbytes); }
__device__ inline uint64_t bloom_hash(const uint64_t* tbl, u128 key, uint32_t nbytes) { return hash_tables_wide(tbl, key, nbytes); }
__device__ inline uint64_t bloom_hash(const uint64_t* tbl, const K256& key, uint32_t nbytes) { return hash_tables_n256(tbl, key, nbytes); }

// the table view of a geometry: what KeyOps' stage_tile, for_each_kmer and text_key look at, and nothing else
__device__ inline DevTable geom_view(const TableGeom& g) { DevTable T; T.g = g; return T; }
__device__ inline WideTable geom_view(const WideGeom& W) { WideTable T; T.W = W; return T; }
__device__ inline NTable geom_view(const NGeom& N) { NTable T; T.N = N; return T; }

template <class Geom>
__global__ __launch_bounds__(kBlock) void bloom_query_ascii_kernel(DevBloom B, Geom G, const uint8_t* __restrict__ base, int64_t lo, int64_t hi,
                                                                   uint64_t* __restrict__ vals, uint8_t* __restrict__ flags) {
  const auto T = geom_view(G);
  typedef typename std::decay<decltype(T)>::type Table;
  typedef KeyOps<Table> K;
  typedef typename K::Key Key;
  __shared__ uint32_t s_codes[kBlock + K::kHaloWords];
  __shared__ uint32_t s_inv[kBlock + K::kHaloWords];
  const uint64_t *t1 = B.tbl1, *t2 = B.tbl2;
  if constexpr(sizeof(Key) == 8) {
    __shared__ uint64_t s_t1[8 * 256];
    __shared__ uint64_t s_t2[8 * 256];
    load_tables_lds(s_t1, B.tbl1, B.nbytes);
    load_tables_lds(s_t2, B.tbl2, B.nbytes);
    t1 = s_t1; t2 = s_t2;
  }
  const bool canonical = K::geom(T).canonical != 0;
  const bool aligned = lo == 0 && (((uintptr_t)vals | (uintptr_t)flags) & 15) == 0;
  const int64_t n_tiles = (hi + kTilePos - 1) / kTilePos;
  for(int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    __syncthreads();
    const typename K::Lane L = K::stage_tile(T, base, tile * kTilePos, lo, hi, s_codes, s_inv);     // contains a barrier
    uint32_t digits = 0, mer = 0, rcm = 0;                        // check() of position j in bits 2j, 2j + 1; a k-mer ends at j, asked as its reverse complement: bit j
    Key prev = Key(); int last = -2; uint32_t d = 0;
    K::for_each_kmer(T, L, [&](int j, const Key& key, bool valid) {
      if(!valid) return;
      if(last != j - 1 || !K::same_key(key, prev)) {              // (a homopolymer's windows share one answer)
        d = bloom_check_ahead(B, bloom_hash(t1, key, B.nbytes), bloom_hash(t2, key, B.nbytes));
        prev = key;
      }
      last = j;
      digits |= d << (2 * j);
      mer |= 1u << j;
      rcm |= ((canonical && !K::same_key(key, K::text_key(T, L, j))) ? 1u : 0u) << j;
    });
    // the flag bytes of positions 4q .. 4q + 3 as one word
    auto flag_word = [&](int q) {
      uint32_t w = 0;
#pragma unroll
      for(int e = 0; e < 4; ++e) {
        const int j = 4 * q + e;
        const uint32_t f = (((mer >> j) & 1u) ? kQMer : 0u) | (((digits >> (2 * j)) & 3u) ? kQFound : 0u) | (((rcm >> j) & 1u) ? kQRevcomp : 0u);
        w |= f << (8 * e);
      }
      return w;
    };
    const int64_t off = tile * kTilePos + 16 * (int64_t)threadIdx.x;       // the lane's first position in the aligned buffer
    if(aligned && off + 16 <= hi) {
#pragma unroll
      for(int q = 0; q < kPerThread / 2; ++q)
        reinterpret_cast<ulonglong2*>(vals + off)[q] = make_ulonglong2((digits >> (4 * q)) & 3u, (digits >> (4 * q + 2)) & 3u);
      if(flags) *reinterpret_cast<uint4*>(flags + off) = make_uint4(flag_word(0), flag_word(1), flag_word(2), flag_word(3));
    } else {
#pragma unroll
      for(int j = 0; j < kPerThread; ++j) {
        const int64_t p = off + j;
        if(p < lo || p >= hi) continue;
        vals[p - lo] = (digits >> (2 * j)) & 3u;
        if(flags) flags[p - lo] = (uint8_t)(flag_word(j >> 2) >> (8 * (j & 3)));
      }
    }
  }
}

}  // namespace jfgpu
