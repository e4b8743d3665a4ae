// jellyfish_amd/csrc/kernels_qtext.hip.hpp -- the lines of `query -s` built from a contract buffer and the answer of a
// query of it (sub_commands/query_main.cc:44-51: `out << *mers << " " << db.check(*mers) << "\n"`; the host form is the loop
// in query_main of jellyfish_amd/cli/jellyfish_amd.cc).
//
// Input: n bases, and vals[p] / flags[p] as jfgpu_query_ascii(_dev) and jfgpu_bc_query_ascii(_dev) write them, all three
// at any alignment (vals on 8 bytes).  Output: for every position p >= k - 1 with JFGPU_Q_MER set, in increasing p, the line
//   KMER COUNT\n
// KMER the k bytes ending at p in upper case (byte & 0xDF), or with JFGPU_Q_REVCOMP their reverse complement, COUNT the
// decimal vals[p].  A line's length is k + 2 + digits(vals[p]), its place the prefix sum of the lengths before it.  The
// structure is that of kernels_text.hip.hpp, a tile of 256 positions per workgroup:
//   qtext_len_kernel    line lengths from flags and vals; bytes and lines of the tile
//   text_scan_kernel    (kernels_text.hip.hpp, as it is) exclusive scan of the tiles' bytes, the two totals
//   qtext_write_kernel  the tile's bases and the k - 1 before them into LDS, at the alignment they have in memory (whole
//                       dwords, bytes at the two ragged ends: nothing outside [0, n) is read); the tile's lines built in
//                       LDS at the alignment they have in the output and copied out as dwords (bytes at the ragged ends)
// A line reads its k bases as aligned LDS dwords shifted into place, four characters at a time; a reverse-complement
// line reads them from the back, swaps the bytes of each dword and complements them.  Three launches, no workgroup waits for
// another.  LDS is dynamic, sized by the host from k (qtext_lds_in / text_lds_out): 256 x (k + 22) bytes of lines, 38 KiB at
// k = 128 and 11 KiB at k = 21.
#pragma once

namespace jfgpu {

struct QTextJob { uint32_t k, line_max; };

// LDS bytes of a tile's bases: up to 3 bytes of misalignment, k - 1 of halo, 256 of the tile, and the dword behind the
// last one that the shifted reads look at
JF_HD uint32_t qtext_lds_in(uint32_t k) { return ((3u + (k - 1u) + (uint32_t)kTextBlock + 3u) & ~3u) + 8u; }

// this lane's position, count and line length (0: no line)
__device__ __forceinline__ uint32_t qtext_line_len(const QTextJob& J, uint64_t n, const uint64_t* __restrict__ vals, const uint8_t* __restrict__ flags,
                                                   uint64_t& val, uint32_t& fl) {
  const uint64_t p = (uint64_t)blockIdx.x * kTextBlock + threadIdx.x;
  val = 0; fl = 0;
  if(p >= n || p + 1 < J.k) return 0;
  fl = flags[p];
  if(!(fl & kQMer)) return 0;
  val = vals[p];
  return J.k + 2u + text_digits(val);
}

// ---- 1. lengths --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTextBlock) void qtext_len_kernel(QTextJob J, uint64_t n, const uint64_t* __restrict__ vals, const uint8_t* __restrict__ flags,
                                                               uint32_t* __restrict__ tile_bytes, uint32_t* __restrict__ tile_kept) {
  __shared__ uint32_t s_w[2 * kTextBlock / 64];
  uint64_t val; uint32_t fl;
  uint32_t len = qtext_line_len(J, n, vals, flags, val, fl);
  uint32_t kept = len != 0;
  text_block_sum2(len, kept, s_w);
  if(threadIdx.x == 0) { tile_bytes[blockIdx.x] = len; tile_kept[blockIdx.x] = kept; }
}

// ---- 3. write ----------------------------------------------------------------------------------------------------------
// four bytes from byte offset `at` of an LDS array of dwords: two aligned reads shifted into place
__device__ __forceinline__ uint32_t qtext_read4(const uint32_t* s, uint32_t at) {
  const uint64_t two = ((uint64_t)s[(at >> 2) + 1] << 32) | s[at >> 2];
  return (uint32_t)(two >> (8u * (at & 3u)));
}
// the complements of four upper-case bases: A <-> T differ by 0x15, C <-> G by 0x04, and bit 1 tells the pairs apart
__device__ __forceinline__ uint32_t qtext_complement4(uint32_t x) {
  const uint32_t cg = (x >> 1) & 0x01010101u;
  return x ^ (cg * 0x04u) ^ ((cg ^ 0x01010101u) * 0x15u);
}

// out + tile_off[tile] is where the tile's text starts; nothing is written when the text of all tiles (totals[0]) does
// not fit cap_bytes.
__global__ __launch_bounds__(kTextBlock) void qtext_write_kernel(QTextJob J, const uint8_t* __restrict__ bases, uint64_t n, const uint64_t* __restrict__ vals,
                                                                 const uint8_t* __restrict__ flags, const uint64_t* __restrict__ tile_off,
                                                                 const uint64_t* __restrict__ totals, uint64_t cap_bytes, uint8_t* __restrict__ out) {
  JF_DYN_LDS(lds);
  __shared__ uint32_t s_w[kTextBlock / 64];
  if(totals[0] > cap_bytes) return;
  const uint32_t lane = threadIdx.x, k = J.k;
  // ---- the tile's bases and their halo: positions [first, last) of the buffer, LDS byte in_mis + (position - first)
  const uint64_t t0 = (uint64_t)blockIdx.x * kTextBlock;
  const uint64_t first = t0 >= k - 1 ? t0 - (k - 1) : 0, last = n - t0 < (uint64_t)kTextBlock ? n : t0 + kTextBlock;
  const uint32_t in_mis = (uint32_t)((uintptr_t)(bases + first) & 3u), in_end = in_mis + (uint32_t)(last - first);
  uint8_t* s_in = (uint8_t*)lds;
  {
    const uint8_t* g = bases + first - in_mis;                     // dword-aligned; byte j of it is LDS byte j, for j in [in_mis, in_end)
    for(uint32_t d = lane; 4 * d < in_end; d += kTextBlock) {
      if(4 * d >= in_mis && 4 * d + 4 <= in_end) ((uint32_t*)s_in)[d] = ((const uint32_t*)g)[d];
      else for(uint32_t j = 4 * d; j < 4 * d + 4; ++j) if(j >= in_mis && j < in_end) s_in[j] = g[j];
    }
  }
  uint8_t* sb = (uint8_t*)lds + qtext_lds_in(k);
  uint64_t val; uint32_t fl;
  const uint32_t len = qtext_line_len(J, n, vals, flags, val, fl);
  // exclusive scan of the lengths: inside the wave by shuffles, across the four waves through LDS
  uint32_t incl = len;
  for(uint32_t o = 1; o < 64u; o <<= 1) { const uint32_t t = __shfl_up(incl, o, 64); if((lane & 63u) >= o) incl += t; }
  if((lane & 63u) == 63u) s_w[lane >> 6] = incl;
  __syncthreads();                                                 // (covers s_in as well)
  uint32_t off = incl - len, total = 0;
  for(uint32_t w = 0; w < (uint32_t)kTextBlock / 64; ++w) { if(w < (lane >> 6)) off += s_w[w]; total += s_w[w]; }
  const uint64_t gbase = tile_off[blockIdx.x];
  const uint32_t mis = (uint32_t)(((uint64_t)(uintptr_t)out + gbase) & 3u);
  if(len) {
    TextEmit E;
    E.begin(sb, mis + off);
    const uint32_t* s32 = (const uint32_t*)s_in;
    const uint32_t w0 = in_mis + (uint32_t)(t0 + lane + 1 - k - first);      // LDS byte of the window's first base
    const uint32_t full = k >> 2, rest = k & 3u, rest_mask = (1u << (8u * rest)) - 1u;
    if(fl & kQRevcomp) {
      for(uint32_t q = 0; q < full; ++q) E.put(qtext_complement4(__builtin_bswap32(qtext_read4(s32, w0 + k - 4u * (q + 1u)) & 0xDFDFDFDFu)), 4u);
      if(rest) E.put(qtext_complement4(__builtin_bswap32(qtext_read4(s32, w0) & 0xDFDFDFDFu) >> (8u * (4u - rest))) & rest_mask, rest);
    } else {
      for(uint32_t q = 0; q < full; ++q) E.put(qtext_read4(s32, w0 + 4u * q) & 0xDFDFDFDFu, 4u);
      if(rest) E.put(qtext_read4(s32, w0 + 4u * full) & 0xDFDFDFDFu & rest_mask, rest);
    }
    E.put(' ', 1u);
    text_put_count(E, val);
    E.put('\n', 1u);
    E.end();
  }
  __syncthreads();
  const uint32_t end = mis + total;                                // LDS byte j is output byte gbase - mis + j, for j in [mis, end)
  uint8_t* g = out + gbase - mis;
  for(uint32_t d = lane; 4 * d < end; d += kTextBlock) {
    if(4 * d >= mis && 4 * d + 4 <= end) ((uint32_t*)g)[d] = ((const uint32_t*)sb)[d];
    else for(uint32_t j = 4 * d; j < 4 * d + 4; ++j) if(j >= mis && j < end) g[j] = sb[j];
  }
}

}  // namespace jfgpu
