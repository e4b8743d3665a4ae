// jellyfish_amd/csrc/kernels_merge.hip.hpp -- k-way merge of sorted databases, one window of positions at a time
// (jellyfish/merge_files.cc:36-176; the host form is do_merge in jellyfish_amd/cli/jellyfish_amd.cc).
//
// Every input is sorted by (pos, key), pos = (M * key) & (size - 1), and equal keys have equal pos, so the records of
// all inputs whose pos lies in [P0, P1) can be merged with no look at the rest.  The host (abi_merge.inl) cuts such a
// window out of every input and uploads the raw record bytes; then
//   merge_decode_kernel   record bytes -> key words, value, pos; flags an input that is not strictly increasing
//   merge_rank_kernel     the place of every record in the union and, at the first input that holds a key, the combined
//                         value (sum / min / max, filter, clamp) or the Jaccard tallies -- rank and scatter, not a sort
//   merge_count_kernel, merge_scan_kernel, merge_pack_kernel
//                         the kept records in rank order as output records; the prefix sum is three launches (per-block
//                         counts, a scan of the block sums, the scatter), no block waits for another
// Keys are KW = 1 to 4 words; comparison is mer_dna::operator<, most significant word first.
#pragma once

namespace jfgpu {

constexpr int kMergeBlock = 256;              // records of a tile = lanes of a workgroup
constexpr uint32_t kMergeMaxInputs = 255;     // the bracket search gives every input a lane of one workgroup
constexpr uint32_t kMergeStage = 1024;        // records of a partner's sub-range staged in LDS (40 KB at four words); longer ones are searched in global memory
constexpr uint32_t kMergeMaxRec = 40;         // 32 key bytes + 8 counter bytes
constexpr uint32_t kMergeBack = 48;           // bytes staged in front of a tile: the record before it (a multiple of 16, >= kMergeMaxRec)
constexpr uint32_t kMergeKeep = 1u << 31;     // out_src: the record is a head that passed the filter

struct MergeSeg {          // one input's share of a window
  uint64_t raw_off;        // byte offset of its first record in the raw buffer (a multiple of 16)
  uint64_t first;          // index of its first record in the decoded arrays
  uint64_t n;              // records
  uint32_t tile0;          // its first tile among the window's tiles (tiles of kMergeBlock records, per input)
  uint32_t rb;             // record bytes: key bytes + this input's counter_len
  uint32_t counter_len;
  uint32_t pad_;
};

struct MergeWin {
  const MergeSeg* segs;
  uint32_t n_inputs, n_tiles;
  uint64_t total;            // records of the window
  uint64_t cap;              // stride of keys[]
  uint64_t* keys;            // [KW][cap], word 0 least significant
  uint64_t* vals;            // [cap]
  uint64_t* pos;             // [cap]
};

template <int KW> struct MKey { uint64_t w[KW]; };

// (pos, key) order: < 0, 0, > 0
template <int KW>
__device__ __forceinline__ int merge_cmp(uint64_t pa, const MKey<KW>& a, uint64_t pb, const MKey<KW>& b) {
  if(pa != pb) return pa < pb ? -1 : 1;
#pragma unroll
  for(int w = KW - 1; w >= 0; --w)
    if(a.w[w] != b.w[w]) return a.w[w] < b.w[w] ? -1 : 1;
  return 0;
}

template <int KW>
__device__ __forceinline__ MKey<KW> merge_load_key(const MergeWin& W, uint64_t i) {
  MKey<KW> k;
#pragma unroll
  for(int w = 0; w < KW; ++w) k.w[w] = W.keys[(uint64_t)w * W.cap + i];
  return k;
}

// the input a tile belongs to: the last one whose first tile is not past it (inputs without records have no tile)
__device__ __forceinline__ uint32_t merge_tile_input(const MergeWin& W, uint32_t tile) {
  uint32_t f = 0;
  for(uint32_t g = 1; g < W.n_inputs; ++g) if(W.segs[g].tile0 <= tile) f = g;
  return f;
}

// 8 bytes at any byte offset of a dword array (LDS): three aligned reads and two funnel shifts
__device__ __forceinline__ uint64_t merge_read64(const uint32_t* s, uint32_t byte_off) {
  const uint32_t a = byte_off >> 2, sh = (byte_off & 3u) * 8u;
  const uint32_t d0 = s[a], d1 = s[a + 1], d2 = s[a + 2];
  return ((uint64_t)funnel_r(d2, d1, sh) << 32) | funnel_r(d1, d0, sh);
}

// M * key through the byte tables, by the product the look-up kernels use (hash_tables, kmer_core.hpp), a key word at a
// time: word w meets the tables of key bytes 8w .. 8w + 7.  fwd == nullptr: the identity matrix
template <int KW>
__device__ __forceinline__ uint64_t merge_pos(const uint64_t* fwd, const MKey<KW>& key, uint32_t kb, uint64_t pos_mask) {
  if(!fwd) return key.w[0] & pos_mask;
  uint64_t p = 0;
#pragma unroll
  for(int w = 0; w < KW; ++w)
    if(kb > 8u * w) p ^= hash_tables(fwd + (size_t)w * 8 * 256, key.w[w], kb - 8u * w < 8u ? kb - 8u * w : 8u);
  return p & pos_mask;
}

// ---- 1. decode -------------------------------------------------------------------------------------------------------
// One workgroup per tile of kMergeBlock records of one input.  The tile's bytes (a multiple of 256 from the segment's
// 16-byte aligned start, so 16-byte aligned themselves) and the 48 bytes in front of them come into LDS as 16-byte loads;
// every lane picks its record out of LDS.  The raw buffer is readable 32 bytes past its last record.
template <int KW>
__global__ __launch_bounds__(kMergeBlock) void merge_decode_kernel(MergeWin W, const uint8_t* __restrict__ raw, const uint64_t* __restrict__ fwd,
                                                                   uint32_t kb, uint32_t key_bits, uint64_t pos_mask, uint32_t* __restrict__ unsorted) {
  __shared__ uint4 s_raw4[(kMergeBack + kMergeBlock * kMergeMaxRec) / 16 + 2];
  __shared__ uint64_t s_key[KW][kMergeBlock + 1];
  __shared__ uint64_t s_pos[kMergeBlock + 1];
  const uint32_t tile = blockIdx.x, lane = threadIdx.x;
  const uint32_t f = merge_tile_input(W, tile);
  const MergeSeg S = W.segs[f];
  const uint64_t i0 = (uint64_t)(tile - S.tile0) * kMergeBlock;
  if(i0 >= S.n) return;                                            // (never: the host counts the tiles)
  const uint32_t cnt = (uint32_t)(S.n - i0 < (uint64_t)kMergeBlock ? S.n - i0 : (uint64_t)kMergeBlock);
  const uint32_t back = i0 ? kMergeBack : 0u;
  const uint32_t n16 = (back + cnt * S.rb + 15u) / 16u + 1u;       // one more: merge_read64 looks up to 11 bytes past a record
  const uint4* src = (const uint4*)(raw + S.raw_off + i0 * S.rb - back);
  for(uint32_t j = lane; j < n16; j += kMergeBlock) s_raw4[j] = src[j];
  __syncthreads();
  const uint32_t* s_raw = (const uint32_t*)s_raw4;
  const uint64_t vmask = S.counter_len >= 8 ? ~0ull : ((1ull << (8 * S.counter_len)) - 1);
  auto decode = [&](uint32_t off, MKey<KW>& key, uint64_t& val) {
#pragma unroll
    for(int w = 0; w < KW; ++w) {
      const int bits = (int)key_bits - 64 * w;                     // bits of the key in this word
      const uint64_t x = bits > 0 ? merge_read64(s_raw, off + 8u * w) : 0ull;
      key.w[w] = bits >= 64 ? x : bits > 0 ? x & ((1ull << bits) - 1) : 0ull;
    }
    val = merge_read64(s_raw, off + kb) & vmask;
  };
  MKey<KW> key; uint64_t val = 0, pos = 0;
  if(lane < cnt) {
    decode(back + lane * S.rb, key, val);
    pos = merge_pos<KW>(fwd, key, kb, pos_mask);
    const uint64_t i = S.first + i0 + lane;
#pragma unroll
    for(int w = 0; w < KW; ++w) { W.keys[(uint64_t)w * W.cap + i] = key.w[w]; s_key[w][lane + 1] = key.w[w]; }
    W.vals[i] = val; W.pos[i] = pos;
    s_pos[lane + 1] = pos;
    if(lane == 0 && back) {                                        // the record in front of the tile
      MKey<KW> pk; uint64_t pv;
      decode(back - S.rb, pk, pv);
#pragma unroll
      for(int w = 0; w < KW; ++w) s_key[w][0] = pk.w[w];
      s_pos[0] = merge_pos<KW>(fwd, pk, kb, pos_mask);
    }
  }
  __syncthreads();
  if(lane < cnt && (lane || back)) {
    MKey<KW> pk;
#pragma unroll
    for(int w = 0; w < KW; ++w) pk.w[w] = s_key[w][lane];
    if(merge_cmp<KW>(s_pos[lane], pk, pos, key) >= 0) atomicOr(&unsorted[f], 1u);
  }
}

// ---- 2. rank and combine ---------------------------------------------------------------------------------------------
// first index in [lo, hi) of the decoded arrays whose record is not smaller than (pos, key) [UPPER: is greater]
template <int KW, bool UPPER>
__device__ __forceinline__ uint64_t merge_bound_global(const MergeWin& W, uint64_t lo, uint64_t hi, uint64_t pos, const MKey<KW>& key) {
  while(lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    const int c = merge_cmp<KW>(W.pos[mid], merge_load_key<KW>(W, mid), pos, key);
    if(UPPER ? c <= 0 : c < 0) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One workgroup per tile of kMergeBlock consecutive records of input f.  Per other input g, one lane brackets the tile:
// [lo_g, hi_g) are g's records not smaller than the tile's first and not greater than its last record.  Everything of g
// before lo_g is smaller than every record of the tile; the place inside the bracket is a search in LDS when the bracket
// fits there (positions are uniform: a bracket is about a tile long) and in global memory when it does not.
//   rank = sum over g of the records of g that are smaller + the number of g < f that hold the key
// The lowest-numbered input that holds a key is its head and combines the values the searches found.  Ranks are below
// W.total whatever the inputs hold: a search answers at most n_g, and n_g - 1 when it found the key.
template <int KW>
__global__ __launch_bounds__(kMergeBlock) void merge_rank_kernel(MergeWin W, int op, uint64_t lower, uint64_t upper, uint64_t vmax,
                                                                 uint64_t* __restrict__ out_val, uint32_t* __restrict__ out_src,
                                                                 unsigned long long* __restrict__ tallies) {
  __shared__ uint64_t s_k[KW][kMergeStage];
  __shared__ uint64_t s_p[kMergeStage];
  __shared__ uint64_t s_lo[kMergeMaxInputs + 1], s_hi[kMergeMaxInputs + 1];
  __shared__ uint64_t s_edge[2][KW + 1];
  __shared__ unsigned long long s_tally[4][kMergeBlock / 64];
  const uint32_t tile = blockIdx.x, lane = threadIdx.x;
  const uint32_t f = merge_tile_input(W, tile);
  const MergeSeg S = W.segs[f];
  const uint64_t i0 = (uint64_t)(tile - S.tile0) * kMergeBlock;
  if(i0 >= S.n) return;
  const uint32_t cnt = (uint32_t)(S.n - i0 < (uint64_t)kMergeBlock ? S.n - i0 : (uint64_t)kMergeBlock);
  const bool live = lane < cnt;
  const uint64_t me = S.first + i0 + (live ? lane : 0u);
  const MKey<KW> key = merge_load_key<KW>(W, me);
  const uint64_t pos = W.pos[me], val = W.vals[me];
  if(lane == 0 || lane == cnt - 1) {
    const int e = lane == 0 ? 0 : 1;
    if(lane == 0 && cnt == 1) {
#pragma unroll
      for(int w = 0; w < KW; ++w) s_edge[1][w] = key.w[w];
      s_edge[1][KW] = pos;
    }
#pragma unroll
    for(int w = 0; w < KW; ++w) s_edge[e][w] = key.w[w];
    s_edge[e][KW] = pos;
  }
  __syncthreads();
  if(lane < W.n_inputs && lane != f) {
    const MergeSeg G = W.segs[lane];
    MKey<KW> a, b;
#pragma unroll
    for(int w = 0; w < KW; ++w) { a.w[w] = s_edge[0][w]; b.w[w] = s_edge[1][w]; }
    const uint64_t lo = merge_bound_global<KW, false>(W, G.first, G.first + G.n, s_edge[0][KW], a);
    const uint64_t hi = merge_bound_global<KW, true>(W, lo, G.first + G.n, s_edge[1][KW], b);
    s_lo[lane] = lo; s_hi[lane] = hi;
  }
  __syncthreads();
  uint64_t rank = i0 + lane, sum = val, minc = val, maxc = val;
  uint32_t present = 1;
  bool head = true;
  for(uint32_t g = 0; g < W.n_inputs; ++g) {
    if(g == f) continue;
    const uint64_t gfirst = W.segs[g].first;
    const uint64_t L = s_lo[g], H = s_hi[g];
    const uint64_t len = H - L;
    uint64_t at;                                                   // index in the decoded arrays of the first record of g that is not smaller
    bool eq = false;
    if(len <= kMergeStage) {
      for(uint32_t j = lane; j < (uint32_t)len; j += kMergeBlock) {
#pragma unroll
        for(int w = 0; w < KW; ++w) s_k[w][j] = W.keys[(uint64_t)w * W.cap + L + j];
        s_p[j] = W.pos[L + j];
      }
      __syncthreads();
      uint32_t lo = 0, hi = (uint32_t)len;
      if(live) {
        while(lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          MKey<KW> m;
#pragma unroll
          for(int w = 0; w < KW; ++w) m.w[w] = s_k[w][mid];
          if(merge_cmp<KW>(s_p[mid], m, pos, key) < 0) lo = mid + 1; else hi = mid;
        }
        if(lo < (uint32_t)len) {
          MKey<KW> m;
#pragma unroll
          for(int w = 0; w < KW; ++w) m.w[w] = s_k[w][lo];
          eq = merge_cmp<KW>(s_p[lo], m, pos, key) == 0;
        }
      }
      at = L + lo;
      __syncthreads();
    } else {
      at = live ? merge_bound_global<KW, false>(W, L, H, pos, key) : L;
      if(live && at < H) eq = merge_cmp<KW>(W.pos[at], merge_load_key<KW>(W, at), pos, key) == 0;
    }
    rank += at - gfirst;
    if(eq) {
      if(g < f) { head = false; ++rank; }
      const uint64_t v = W.vals[at];
      sum += v; minc = v < minc ? v : minc; maxc = v > maxc ? v : maxc; ++present;
    }
  }
  if(present < W.n_inputs) minc = 0;                               // absent from some input: count 0 there
  unsigned long long t0 = 0, t1 = 0, t2 = 0, t3 = 0;
  if(live) {
    if(op != 3) {
      const uint64_t v = op == 0 ? sum : op == 1 ? minc : maxc;
      const bool keep = head && v >= lower && v <= upper;          // the filter sees the unclamped value
      out_val[rank] = v < vmax ? v : vmax;
      out_src[rank] = (uint32_t)me | (keep ? kMergeKeep : 0u);
    } else if(head) { t0 = minc > 0; t1 = minc; t2 = 1; t3 = maxc; }
  }
  if(op == 3) {                                                    // Jaccard: four tallies, one atomic each per workgroup
    for(int o = 32; o > 0; o >>= 1) {
      t0 += __shfl_down(t0, o, 64); t1 += __shfl_down(t1, o, 64); t2 += __shfl_down(t2, o, 64); t3 += __shfl_down(t3, o, 64);
    }
    if((lane & 63) == 0) { s_tally[0][lane >> 6] = t0; s_tally[1][lane >> 6] = t1; s_tally[2][lane >> 6] = t2; s_tally[3][lane >> 6] = t3; }
    __syncthreads();
    if(lane < 4) {
      unsigned long long t = 0;
      for(int w = 0; w < kMergeBlock / 64; ++w) t += s_tally[lane][w];
      if(t) atomicAdd(&tallies[lane], t);
    }
  }
}

// ---- 3. compact and pack ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMergeBlock) void merge_count_kernel(const uint32_t* __restrict__ out_src, uint64_t total, uint32_t* __restrict__ block_cnt) {
  __shared__ uint32_t s_w[kMergeBlock / 64];
  const uint64_t r = (uint64_t)blockIdx.x * kMergeBlock + threadIdx.x;
  const bool keep = r < total && (out_src[r] & kMergeKeep);
  const uint32_t c = (uint32_t)__popcll(__ballot(keep));
  if((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
  __syncthreads();
  if(threadIdx.x == 0) { uint32_t t = 0; for(int w = 0; w < kMergeBlock / 64; ++w) t += s_w[w]; block_cnt[blockIdx.x] = t; }
}

// exclusive scan of the block counts by one workgroup, a chunk of kMergeBlock at a time; n_kept[0] = their sum
__global__ __launch_bounds__(kMergeBlock) void merge_scan_kernel(const uint32_t* __restrict__ block_cnt, uint32_t nb, uint64_t* __restrict__ block_off, uint64_t* __restrict__ n_kept) {
  __shared__ uint64_t s_x[kMergeBlock];
  uint64_t carry = 0;
  for(uint32_t base = 0; base < nb; base += kMergeBlock) {
    const uint32_t i = base + threadIdx.x;
    const uint64_t mine = i < nb ? block_cnt[i] : 0;
    s_x[threadIdx.x] = mine;
    __syncthreads();
    for(uint32_t o = 1; o < (uint32_t)kMergeBlock; o <<= 1) {
      const uint64_t add = threadIdx.x >= o ? s_x[threadIdx.x - o] : 0;
      __syncthreads();
      s_x[threadIdx.x] += add;
      __syncthreads();
    }
    if(i < nb) block_off[i] = carry + s_x[threadIdx.x] - mine;
    carry += s_x[kMergeBlock - 1];
    __syncthreads();
  }
  if(threadIdx.x == 0) n_kept[0] = carry;
}

// The kept records of a block of ranks, as output records (kb key bytes, ocl value bytes), put together in LDS at the
// alignment they have in the output and copied out as dwords (bytes at the two ragged ends).
template <int KW>
__global__ __launch_bounds__(kMergeBlock) void merge_pack_kernel(MergeWin W, const uint64_t* __restrict__ out_val, const uint32_t* __restrict__ out_src,
                                                                 const uint64_t* __restrict__ block_off, uint32_t kb, uint32_t ocl, uint8_t* __restrict__ out) {
  __shared__ uint32_t s_out[(kMergeBlock * kMergeMaxRec) / 4 + 2];
  __shared__ uint32_t s_w[kMergeBlock / 64];
  const uint32_t lane = threadIdx.x, orb = kb + ocl;
  const uint64_t r = (uint64_t)blockIdx.x * kMergeBlock + lane;
  uint32_t src = r < W.total ? out_src[r] : 0u;
  const bool keep = (src & kMergeKeep) && (uint64_t)(src & ~kMergeKeep) < W.total;
  src &= ~kMergeKeep;
  const unsigned long long bal = __ballot(keep);
  if((lane & 63) == 0) s_w[lane >> 6] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t idx = (uint32_t)__popcll(bal & ((1ull << (lane & 63)) - 1)), kept = 0;
  for(uint32_t w = 0; w < (uint32_t)kMergeBlock / 64; ++w) { if(w < (lane >> 6)) idx += s_w[w]; kept += s_w[w]; }
  const uint64_t gbase = block_off[blockIdx.x] * orb;
  const uint32_t mis = (uint32_t)(gbase & 3u);
  uint8_t* sb = (uint8_t*)s_out;
  if(keep) {
    const MKey<KW> key = merge_load_key<KW>(W, src);
    const uint64_t v = out_val[r];
    uint8_t* p = sb + mis + idx * orb;
#pragma unroll
    for(int w = 0; w < KW; ++w)
      for(uint32_t b = 0; b < 8 && 8u * w + b < kb; ++b) p[8 * w + b] = (uint8_t)(key.w[w] >> (8 * b));
    for(uint32_t b = 0; b < ocl; ++b) p[kb + b] = (uint8_t)(v >> (8 * b));
  }
  __syncthreads();
  const uint32_t end = mis + kept * orb;                           // LDS byte j is output byte gbase - mis + j, for j in [mis, end)
  uint8_t* g = out + (gbase - mis);
  for(uint32_t d = lane; 4 * d < end; d += kMergeBlock) {
    if(4 * d >= mis && 4 * d + 4 <= end) ((uint32_t*)g)[d] = s_out[d];
    else for(uint32_t j = 4 * d; j < 4 * d + 4; ++j) if(j >= mis && j < end) g[j] = sb[j];
  }
}

}  // namespace jfgpu
