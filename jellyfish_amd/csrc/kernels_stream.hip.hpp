// jellyfish_amd/csrc/kernels_stream.hip.hpp -- where an inflated FASTA / FASTQ stream may be cut, on the device (gfx950).
//
// bgzip-compressed sequence files exist as text only in device memory (kernels_bgzf.hip.hpp inflates them), so the cut
// the host makes for plain files (device_parser.hpp: memrchr for FASTA, fastq_cut_in for FASTQ) is made here:
//
//   stream_cut_kernel   S[0, len) and a format -> the length of the longest prefix the parse kernels take as a chunk
//                       (kernels_parse.hip.hpp), 0 when there is none
//     FASTA  1 + the position of the last '\n'
//     FASTQ  the largest s with 0 < s < len, S[s-1] == '\n', S[s] == '@' and, e1 being the first '\n' at or after s and
//            e2 the first one after e1, e2 + 1 < len and S[e2+1] == '+' (a quality line may start with '@', but then
//            its second-next line is a sequence line): fastq_cut_in's rule with no limit on the lines looked at
//
// One workgroup walks the stream backwards in aligned tiles of 4096 bytes, 16 bytes a lane.  Per tile the newline
// positions are compacted into LDS in ascending order (ballot-free: a popcount per lane, one workgroup scan), so "the
// first newline at or after s" is the entry whose index is the number of newlines before s, and the second-next one is
// the entry after it.  The two nearest newlines of the tiles already walked are carried in registers and stand behind
// the tile's list.  The walk stops at the first tile that yields a cut: for short reads that is the first one, a read
// of many tiles takes as many rounds and gives the same answer.  Nothing is read at or beyond len rounded up to 16.
#pragma once
#include "kernels_parse.hip.hpp"

namespace jfgpu {

constexpr int kCutBlock = 256;
constexpr int kCutLane = 16;                             // bytes per thread, one 16-byte load
constexpr int kCutTile = kCutBlock * kCutLane;           // 4096 bytes per round
constexpr uint64_t kCutNone = ~0ull;

// S must be 16-byte aligned and readable up to len rounded up to 16 bytes.
__global__ __launch_bounds__(kCutBlock) void stream_cut_kernel(const uint8_t* __restrict__ S, uint64_t len, uint32_t fmt,
                                                               unsigned long long* __restrict__ cut) {
  __shared__ uint16_t s_nl[kCutTile];                    // the tile's newlines, tile-relative, ascending
  __shared__ uint32_t s_w[kCutBlock / 64];
  __shared__ unsigned long long s_best[kCutBlock / 64];
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint64_t c1 = kCutNone, c2 = kCutNone;                 // first and second newline of the tiles already walked
  unsigned long long found = 0;
  for(int64_t tile = len ? (int64_t)((len - 1) / kCutTile) : -1; tile >= 0; --tile) {
    const uint64_t base = (uint64_t)tile * kCutTile, p0 = base + (uint64_t)t * kCutLane;
    uint4 w = make_uint4(0, 0, 0, 0);
    uint32_t nl = 0, at = 0;
    if(p0 < len) {
      w = *reinterpret_cast<const uint4*>(S + p0);
      const uint32_t valid = len - p0 >= (uint64_t)kCutLane ? 0xFFFFu : (1u << (uint32_t)(len - p0)) - 1u;
#pragma unroll
      for(int i = 0; i < kCutLane; ++i) {
        const uint32_t c = byte_of(w, i);
        if(c == '\n') nl |= 1u << i;
        if(c == '@') at |= 1u << i;
      }
      nl &= valid; at &= valid;
    }
    uint32_t m = 0;                                      // newlines in the tile
    const uint32_t before = block_scan_sum<uint32_t>((uint32_t)__popc(nl), s_w, &m);
    unsigned long long best = 0;                         // (a cut is never 0)
    if(fmt == PARSE_FASTA) {
      if(nl) best = p0 + (uint64_t)(31 - __clz((int)nl)) + 1;
    } else {
      { uint32_t r = before;
        for(uint32_t b = nl; b; b &= b - 1) s_nl[r++] = (uint16_t)(t * kCutLane + (uint32_t)__ffs((int)b) - 1); }
      __syncthreads();
      // candidates: '@' right after a '\n' (the byte before this lane's first one is read from the stream)
      uint32_t cand = at & (nl << 1);
      if((at & 1u) && p0 > 0 && S[p0 - 1] == '\n') cand |= 1u;
      while(cand && !best) {                             // from the last one down
        const int i = 31 - __clz((int)cand);
        cand &= ~(1u << i);
        const uint32_t r = before + (uint32_t)__popc(nl & ((1u << i) - 1u));      // newlines of the tile before s
        uint64_t e2;
        if(r + 1 < m) e2 = base + s_nl[r + 1];
        else e2 = r < m ? c1 : c2;
        if(e2 != kCutNone && e2 + 1 < len && S[e2 + 1] == '+') best = p0 + (uint64_t)i;
      }
    }
    for(int o = 32; o; o >>= 1) { const unsigned long long x = __shfl_xor(best, o, 64); best = x > best ? x : best; }
    if(lane == 0) s_best[wave] = best;
    __syncthreads();
    for(uint32_t k = 0; k < kCutBlock / 64; ++k) found = s_best[k] > found ? s_best[k] : found;
    if(found) break;                                     // (the same value in every thread)
    if(fmt != PARSE_FASTA) {
      if(m >= 2) { c1 = base + s_nl[0]; c2 = base + s_nl[1]; }
      else if(m == 1) { c2 = c1; c1 = base + s_nl[0]; }
    }
    __syncthreads();                                     // s_nl and s_best are written again in the next round
  }
  if(t == 0) *cut = found;
}

}  // namespace jfgpu
