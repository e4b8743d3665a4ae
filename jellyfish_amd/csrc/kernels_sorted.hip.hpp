// jellyfish_amd/csrc/kernels_sorted.hip.hpp -- query: look-ups in the packed records of a binary/sorted database as the file has them
// (include/jellyfish/binary_dumper.hpp:112-213 binary_query; sub_commands/query_main.cc:44-51 query_from_sequence).
//
// The records of such a file ascend by (pos, key), pos = (M * key) & (size - 1), and the positions of hashed keys are uniform:
// the file is its own index.  The body is uploaded unchanged and
//   sorted_index_kernel        cuts it into 2^B buckets by the top B bits of pos: index[b] is the first record whose bucket is
//                              not below b, index[2^B] = n.  It also flags a body that is not strictly increasing
//   sorted_longest_kernel      the longest bucket, for jfgpu_sorted_info
//   sorted_query_ascii_kernel  every k-mer of a contract buffer, rolled and made canonical over KeyOps like bloom_query_ascii_kernel,
//                              hashed through the header's byte tables and answered by a scan of its bucket
//   sorted_lookup_kernel       the same scan for encoded keys (kw words each, as jfgpu_lookup)
// A scan compares keys for equality and nothing else: it does not hash a record and does not care in which order a bucket's
// records come.  Records are kb = ceil(2k / 8) key bytes and vb counter bytes at any byte alignment; the body is readable
// 32 bytes past its last record.  Nothing here writes the body: no atomics but the order flag and the longest bucket.
#pragma once

namespace jfgpu {

struct SortedView {
  const uint8_t* body;       // n_records records of rb bytes from a 16-byte boundary
  uint64_t* index;           // [2^B + 1]
  const uint64_t* fwd;       // the matrix's byte tables [kb][256]; nullptr: the identity matrix
  uint64_t n_records;
  uint64_t pos_mask;         // size - 1
  uint64_t val_mask;         // 2^(8 vb) - 1
  uint32_t rb, kb, key_bits;
  uint32_t bucket_shift;     // lsize - B: bucket = pos >> bucket_shift
};

// the bits of a key that lie in its word w, as a mask of that word
__device__ __forceinline__ uint64_t sorted_word_mask(uint32_t key_bits, int w) {
  const int bits = (int)key_bits - 64 * w;
  return bits >= 64 ? ~0ull : bits > 0 ? ((1ull << bits) - 1) : 0ull;
}

// 8 bytes at any byte offset of the body: merge_read64 on global memory
__device__ __forceinline__ uint64_t sorted_read64(const uint32_t* __restrict__ g, uint64_t byte_off) {
  const uint64_t a = byte_off >> 2;
  const uint32_t sh = ((uint32_t)byte_off & 3u) * 8u;
  const uint32_t d0 = g[a], d1 = g[a + 1], d2 = g[a + 2];
  return ((uint64_t)funnel_r(d2, d1, sh) << 32) | funnel_r(d1, d0, sh);
}

// ---- 1. the bucket index ----------------------------------------------------------------------------------------------
// One workgroup per tile of kMergeBlock records, staged like merge_decode_kernel: the tile's bytes (a multiple of 256 from the
// body's start, so 16-byte aligned) and the 48 bytes in front of them as 16-byte loads into LDS, a lane picks its record
// with merge_read64.  Record i whose bucket is above record i - 1's writes index[b] = i for every b in between: every entry
// has one writer.  A body out of order leaves entries unwritten; it is refused by the host, which reads the flag.
template <int KW>
__global__ __launch_bounds__(kMergeBlock) void sorted_index_kernel(SortedView S, uint64_t n_buckets, uint32_t* __restrict__ unsorted) {
  __shared__ uint4 s_raw4[(kMergeBack + kMergeBlock * kMergeMaxRec) / 16 + 2];
  __shared__ uint64_t s_key[KW][kMergeBlock + 1];
  __shared__ uint64_t s_pos[kMergeBlock + 1];
  const uint32_t lane = threadIdx.x;
  const uint64_t i0 = (uint64_t)blockIdx.x * kMergeBlock;
  if(i0 >= S.n_records) return;                                    // (never: the host counts the tiles)
  const uint32_t cnt = (uint32_t)(S.n_records - i0 < (uint64_t)kMergeBlock ? S.n_records - i0 : (uint64_t)kMergeBlock);
  const uint32_t back = i0 ? kMergeBack : 0u;
  const uint32_t n16 = (back + cnt * S.rb + 15u) / 16u + 1u;       // one more: merge_read64 looks up to 11 bytes past a record
  const uint4* src = (const uint4*)(S.body + i0 * S.rb - back);
  for(uint32_t j = lane; j < n16; j += kMergeBlock) s_raw4[j] = src[j];
  __syncthreads();
  const uint32_t* s_raw = (const uint32_t*)s_raw4;
  auto decode = [&](uint32_t off, MKey<KW>& key) {
#pragma unroll
    for(int w = 0; w < KW; ++w) {
      const uint64_t m = sorted_word_mask(S.key_bits, w);
      key.w[w] = m ? merge_read64(s_raw, off + 8u * w) & m : 0ull;
    }
  };
  MKey<KW> key; uint64_t pos = 0;
  if(lane < cnt) {
    decode(back + lane * S.rb, key);
    pos = merge_pos<KW>(S.fwd, key, S.kb, S.pos_mask);
#pragma unroll
    for(int w = 0; w < KW; ++w) s_key[w][lane + 1] = key.w[w];
    s_pos[lane + 1] = pos;
    if(lane == 0 && back) {                                        // the record in front of the tile
      MKey<KW> pk;
      decode(back - S.rb, pk);
#pragma unroll
      for(int w = 0; w < KW; ++w) s_key[w][0] = pk.w[w];
      s_pos[0] = merge_pos<KW>(S.fwd, pk, S.kb, S.pos_mask);
    }
  }
  __syncthreads();
  if(lane >= cnt) return;
  const uint64_t i = i0 + lane, bucket = pos >> S.bucket_shift;    // bucket < n_buckets: pos <= pos_mask
  uint64_t from = 0;                                               // the first entry this record writes
  if(lane || back) {
    MKey<KW> pk;
#pragma unroll
    for(int w = 0; w < KW; ++w) pk.w[w] = s_key[w][lane];
    if(merge_cmp<KW>(s_pos[lane], pk, pos, key) >= 0) atomicOr(unsorted, 1u);
    from = (s_pos[lane] >> S.bucket_shift) + 1;
  }
  for(uint64_t b = from; b <= bucket; ++b) S.index[b] = i;
  if(i == S.n_records - 1)
    for(uint64_t b = bucket + 1; b <= n_buckets; ++b) S.index[b] = S.n_records;
}

// max over b of index[b + 1] - index[b], into longest[0] (zeroed by the host)
__global__ __launch_bounds__(kMergeBlock) void sorted_longest_kernel(const uint64_t* __restrict__ index, uint64_t n_buckets, unsigned long long* __restrict__ longest) {
  unsigned long long m = 0;
  for(uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_buckets; b += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t lo = index[b], hi = index[b + 1];
    const unsigned long long len = hi > lo ? hi - lo : 0;
    m = len > m ? len : m;
  }
  for(int o = 32; o > 0; o >>= 1) { const unsigned long long x = __shfl_down(m, o, 64); m = x > m ? x : m; }
  if((threadIdx.x & 63) == 0 && m) atomicMax(longest, m);
}

// ---- 2. the bucket scan -----------------------------------------------------------------------------------------------
// The count of `key` (NW words, clean above key_bits) at position pos, or false.  The first key word decides for nearly every
// record; the other words and the count are read only behind it.  A bucket's end is clamped to the body.
template <int NW>
__device__ __forceinline__ bool sorted_scan(const SortedView& S, uint64_t pos, const uint64_t (&key)[NW], uint64_t& val) {
  const uint64_t b = pos >> S.bucket_shift;
  uint64_t r = S.index[b], hi = S.index[b + 1];
  if(hi > S.n_records) hi = S.n_records;
  const uint32_t* __restrict__ body = (const uint32_t*)S.body;
  const uint64_t m0 = sorted_word_mask(S.key_bits, 0);
  for(; r < hi; ++r) {
    const uint64_t off = r * S.rb;
    if((sorted_read64(body, off) & m0) != key[0]) continue;
    bool eq = true;
#pragma unroll
    for(int w = 1; w < NW; ++w) {
      const uint64_t m = sorted_word_mask(S.key_bits, w);
      if(m) eq = eq && (sorted_read64(body, off + 8u * w) & m) == key[w];
    }
    if(!eq) continue;
    val = sorted_read64(body, off + S.kb) & S.val_mask;
    return true;
  }
  return false;
}

__device__ __forceinline__ void sorted_words(uint64_t key, uint64_t (&w)[1]) { w[0] = key; }
__device__ __forceinline__ void sorted_words(u128 key, uint64_t (&w)[2]) { w[0] = (uint64_t)key; w[1] = (uint64_t)(key >> 64); }
__device__ __forceinline__ void sorted_words(const K256& key, uint64_t (&w)[4]) { w[0] = key.w[0]; w[1] = key.w[1]; w[2] = key.w[2]; w[3] = key.w[3]; }

// ---- 3. every k-mer of a contract buffer ------------------------------------------------------------------------------
// The skeleton of bloom_query_ascii_kernel with the answer of query_ascii_kernel: vals[p] and flags[p] indexed by the position
// of the window's last base, every entry of [0, hi - lo) written, nothing else.  One-word keys stage the byte tables in LDS.
template <class Geom>
__global__ __launch_bounds__(kBlock) void sorted_query_ascii_kernel(SortedView S, Geom G, const uint8_t* __restrict__ base, int64_t lo, int64_t hi,
                                                                    uint64_t* __restrict__ vals, uint8_t* __restrict__ flags) {
  const auto T = geom_view(G);
  typedef typename std::decay<decltype(T)>::type Table;
  typedef KeyOps<Table> K;
  typedef typename K::Key Key;
  constexpr int NW = sizeof(Key) / 8;
  __shared__ uint32_t s_codes[kBlock + K::kHaloWords];
  __shared__ uint32_t s_inv[kBlock + K::kHaloWords];
  const uint64_t* fwd = S.fwd;
  if constexpr(NW == 1) {
    __shared__ uint64_t s_fwd[8 * 256];
    if(S.fwd) { load_tables_lds(s_fwd, S.fwd, S.kb); fwd = s_fwd; }
  }
  const bool canonical = K::geom(T).canonical != 0;
  const bool aligned = lo == 0 && (((uintptr_t)vals | (uintptr_t)flags) & 15) == 0;
  const int64_t n_tiles = (hi + kTilePos - 1) / kTilePos;
  for(int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    __syncthreads();
    const typename K::Lane L = K::stage_tile(T, base, tile * kTilePos, lo, hi, s_codes, s_inv);     // contains a barrier
    // indexed by the unrolled position j (compile-time after unrolling) so these stay in VGPRs
    uint64_t v[kPerThread]; uint32_t fl[kPerThread / 4] = {0, 0, 0, 0};
#pragma unroll
    for(int j = 0; j < kPerThread; ++j) v[j] = 0;
    Key prev = Key(); int last = -2; uint64_t count = 0; uint32_t bits = 0;
    K::for_each_kmer(T, L, [&](int j, const Key& key, bool valid) {
      if(!valid) return;
      if(last != j - 1 || !K::same_key(key, prev)) {              // (a homopolymer's windows share one answer)
        uint64_t w[NW];
        sorted_words(key, w);
        const uint64_t pos = (fwd ? bloom_hash(fwd, key, S.kb) : w[0]) & S.pos_mask;
        count = 0;
        bits = sorted_scan<NW>(S, pos, w, count) ? kQFound : 0u;
        prev = key;
      }
      last = j;
      v[j] = count;
      fl[j >> 2] |= (kQMer | bits | ((canonical && !K::same_key(key, K::text_key(T, L, j))) ? kQRevcomp : 0u)) << (8 * (j & 3));
    });
    const int64_t off = tile * kTilePos + 16 * (int64_t)threadIdx.x;       // the lane's first position in the aligned buffer
    if(aligned && off + 16 <= hi) {
#pragma unroll
      for(int q = 0; q < kPerThread / 2; ++q) reinterpret_cast<ulonglong2*>(vals + off)[q] = make_ulonglong2(v[2 * q], v[2 * q + 1]);
      if(flags) *reinterpret_cast<uint4*>(flags + off) = make_uint4(fl[0], fl[1], fl[2], fl[3]);
    } else {
#pragma unroll
      for(int j = 0; j < kPerThread; ++j) {
        const int64_t p = off + j;
        if(p < lo || p >= hi) continue;
        vals[p - lo] = v[j];
        if(flags) flags[p - lo] = (uint8_t)(fl[j >> 2] >> (8 * (j & 3)));
      }
    }
  }
}

// ---- 4. encoded keys --------------------------------------------------------------------------------------------------
// keys: KW little-endian words each, bits above 2k ignored (jfgpu_lookup)
template <int KW>
__global__ __launch_bounds__(kBlock) void sorted_lookup_kernel(SortedView S, const uint64_t* __restrict__ keys, uint64_t n,
                                                               uint64_t* __restrict__ vals, uint8_t* __restrict__ found) {
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    MKey<KW> key;
#pragma unroll
    for(int w = 0; w < KW; ++w) key.w[w] = keys[i * KW + w] & sorted_word_mask(S.key_bits, w);
    uint64_t count = 0;
    const bool hit = sorted_scan<KW>(S, merge_pos<KW>(S.fwd, key, S.kb, S.pos_mask), key.w, count);
    vals[i] = count;
    if(found) found[i] = hit;
  }
}

}  // namespace jfgpu
