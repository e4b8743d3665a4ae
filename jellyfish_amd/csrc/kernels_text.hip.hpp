// jellyfish_amd/csrc/kernels_text.hip.hpp -- binary/sorted records formatted as text, a tile of records per workgroup
// (sub_commands/dump_main.cc:35-52; the host forms are dump_main in jellyfish_amd/cli/jellyfish_amd.cc and
// write_text_records in jellyfish_amd/include/jellyfish_amd/dumpers.hpp).
//
// Input: n packed records (kb = (2k+7)/8 key bytes, vb count bytes, both little endian) from a 16-byte boundary.  Output:
// the lines of the records whose count lies in [lower, upper], in input order,
//   column   KMER<sep>COUNT\n          FASTA   >COUNT\nKMER\n
// KMER as mer_dna::to_str (character i is "ACGT"[(key >> 2(k-1-i)) & 3]; bits of the top key byte above 2k are not looked
// at), COUNT as the decimal uint64.  A line's length is k + 2 + digits(count) (+ 1 for FASTA), its place the prefix sum of
// the lengths before it:
//   text_len_kernel     a tile's bytes into LDS as 16-byte loads; count, filter, line length; bytes and lines of the tile
//   text_scan_kernel    exclusive scan of the tiles' bytes by one workgroup (64-bit offsets), the two totals
//   text_write_kernel   the tile's lines built in LDS at the alignment they have in the output, copied out as dwords
//                       (bytes at the two ragged ends)
// Three launches, no workgroup waits for another.  LDS is dynamic, sized by the host from the record and line lengths of
// the job (text_lds_raw / text_lds_out), so that short mers are not held to the occupancy of k = 128.
#pragma once

namespace jfgpu {

constexpr int kTextBlock = 256;               // records of a tile = lanes of a workgroup
constexpr uint32_t kTextColumn = 0, kTextFasta = 1;

struct TextJob {
  uint32_t k, kb, vb, rb;                     // mer length, key bytes, count bytes, record bytes
  uint32_t layout, sep;                       // kTextColumn / kTextFasta; the column separator
  uint32_t line_max;                          // longest line of the job: sizes the LDS of text_write_kernel
  uint32_t pad_;
  uint64_t lower, upper;
};

// LDS bytes of a tile's records (merge_read64 looks up to 11 bytes past a record's count) and of its lines (up to three
// bytes of the line in front share the first dword)
JF_HD uint32_t text_lds_raw(uint32_t rb) { return (((uint32_t)kTextBlock * rb + 15u) & ~15u) + 16u; }
JF_HD uint32_t text_lds_out(uint32_t line_max) { return (((uint32_t)kTextBlock * line_max + 3u) & ~3u) + 8u; }

JF_HD uint32_t text_digits32(uint32_t v) {
  return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u
       : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
// decimal digits of v; counts below 2^32 never touch 64-bit compares
JF_HD uint32_t text_digits(uint64_t v) {
  if(!(v >> 32)) return text_digits32((uint32_t)v);
  return v < 10000000000ull ? 10u : v < 100000000000ull ? 11u : v < 1000000000000ull ? 12u : v < 10000000000000ull ? 13u
       : v < 100000000000000ull ? 14u : v < 1000000000000000ull ? 15u : v < 10000000000000000ull ? 16u
       : v < 100000000000000000ull ? 17u : v < 1000000000000000000ull ? 18u : v < 10000000000000000000ull ? 19u : 20u;
}

// the tile's record bytes into LDS; returns its records.  Reads up to the 16-byte boundary behind the tile's last record.
__device__ __forceinline__ uint32_t text_stage(const uint8_t* __restrict__ raw, uint64_t n, uint32_t rb, uint4* s_raw4) {
  const uint64_t i0 = (uint64_t)blockIdx.x * kTextBlock;
  const uint32_t cnt = (uint32_t)(n - i0 < (uint64_t)kTextBlock ? n - i0 : (uint64_t)kTextBlock);
  const uint32_t n16 = (cnt * rb + 15u) / 16u;
  const uint4* src = (const uint4*)(raw + i0 * rb);
  for(uint32_t j = threadIdx.x; j < n16; j += kTextBlock) s_raw4[j] = src[j];
  __syncthreads();
  return cnt;
}

// this lane's count, and the length of its line (0: no record, or one the filter drops)
__device__ __forceinline__ uint32_t text_line_len(const TextJob& J, const uint32_t* s_raw, uint32_t cnt, uint64_t& val) {
  const uint32_t lane = threadIdx.x;
  val = 0;
  if(lane >= cnt) return 0;
  const uint64_t vmask = J.vb >= 8 ? ~0ull : ((1ull << (8 * J.vb)) - 1);
  val = merge_read64(s_raw, lane * J.rb + J.kb) & vmask;
  if(val < J.lower || val > J.upper) return 0;
  return J.k + 2u + text_digits(val) + (J.layout == kTextFasta ? 1u : 0u);
}

// sum over the workgroup of a and of b (every lane gets both); s_w: 2 * kTextBlock / 64 words
__device__ __forceinline__ void text_block_sum2(uint32_t& a, uint32_t& b, uint32_t* s_w) {
  for(int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
  if((threadIdx.x & 63) == 0) { s_w[threadIdx.x >> 6] = a; s_w[kTextBlock / 64 + (threadIdx.x >> 6)] = b; }
  __syncthreads();
  a = b = 0;
  for(int w = 0; w < kTextBlock / 64; ++w) { a += s_w[w]; b += s_w[kTextBlock / 64 + w]; }
}

// ---- 1. lengths --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTextBlock) void text_len_kernel(TextJob J, const uint8_t* __restrict__ raw, uint64_t n,
                                                              uint32_t* __restrict__ tile_bytes, uint32_t* __restrict__ tile_kept) {
  JF_DYN_LDS(lds);
  __shared__ uint32_t s_w[2 * kTextBlock / 64];
  const uint32_t cnt = text_stage(raw, n, J.rb, (uint4*)lds);
  uint64_t val;
  uint32_t len = text_line_len(J, (const uint32_t*)lds, cnt, val);
  uint32_t kept = len != 0;
  text_block_sum2(len, kept, s_w);
  if(threadIdx.x == 0) { tile_bytes[blockIdx.x] = len; tile_kept[blockIdx.x] = kept; }
}

// ---- 2. scan -----------------------------------------------------------------------------------------------------------
// exclusive scan of the tiles' bytes by one workgroup, a chunk of kTextBlock at a time; totals = {bytes, lines}
__global__ __launch_bounds__(kTextBlock) void text_scan_kernel(const uint32_t* __restrict__ tile_bytes, const uint32_t* __restrict__ tile_kept, uint32_t nb,
                                                               uint64_t* __restrict__ tile_off, uint64_t* __restrict__ totals) {
  __shared__ uint64_t s_x[kTextBlock];
  __shared__ uint64_t s_k[kTextBlock / 64];
  uint64_t carry = 0, kept = 0;
  for(uint32_t base = 0; base < nb; base += kTextBlock) {
    const uint32_t i = base + threadIdx.x;
    const uint64_t mine = i < nb ? tile_bytes[i] : 0;
    kept += i < nb ? tile_kept[i] : 0;
    s_x[threadIdx.x] = mine;
    __syncthreads();
    for(uint32_t o = 1; o < (uint32_t)kTextBlock; o <<= 1) {
      const uint64_t add = threadIdx.x >= o ? s_x[threadIdx.x - o] : 0;
      __syncthreads();
      s_x[threadIdx.x] += add;
      __syncthreads();
    }
    if(i < nb) tile_off[i] = carry + s_x[threadIdx.x] - mine;
    carry += s_x[kTextBlock - 1];
    __syncthreads();
  }
  for(int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o, 64);
  if((threadIdx.x & 63) == 0) s_k[threadIdx.x >> 6] = kept;
  __syncthreads();
  if(threadIdx.x == 0) {
    uint64_t t = 0;
    for(int w = 0; w < kTextBlock / 64; ++w) t += s_k[w];
    totals[0] = carry; totals[1] = t;
  }
}

// ---- 3. write ----------------------------------------------------------------------------------------------------------
// A line under construction in LDS.  Bytes gather in a register and leave as whole dwords; only the line's first and last
// dword, which it may share with its neighbours, are stored byte by byte.
struct TextEmit {
  uint8_t* sb;             // the tile's lines
  uint32_t d;              // dword being filled
  uint32_t fill;           // bytes of acc that are placed (those of the line in front included)
  uint32_t lead;           // bytes of the first dword that belong to the line in front (0 once that dword is out)
  uint64_t acc;
  __device__ __forceinline__ void begin(uint8_t* base, uint32_t at) { sb = base; d = at >> 2; fill = lead = at & 3u; acc = 0; }
  // the n <= 4 low bytes of c, which is zero above them
  __device__ __forceinline__ void put(uint32_t c, uint32_t n) {
    acc |= (uint64_t)c << (8u * fill);
    fill += n;
    if(fill >= 4u) {
      const uint32_t w = (uint32_t)acc;
      if(lead) { for(uint32_t j = lead; j < 4u; ++j) sb[4u * d + j] = (uint8_t)(w >> (8u * j)); lead = 0; }
      else ((uint32_t*)sb)[d] = w;
      ++d; acc >>= 32; fill -= 4u;
    }
  }
  __device__ __forceinline__ void end() {
    for(uint32_t j = lead; j < fill; ++j) sb[4u * d + j] = (uint8_t)((uint32_t)acc >> (8u * j));
  }
};

// four decimal digits of y < 10^4 as characters, the most significant in the low byte
__device__ __forceinline__ uint32_t text_chars4(uint32_t y) {
  const uint32_t hi = y / 100u, lo = y - hi * 100u;
  const uint32_t a = hi / 10u, b = hi - a * 10u, c = lo / 10u, e = lo - c * 10u;
  return 0x30303030u + (a | (b << 8) | (c << 16) | (e << 24));
}

// `have` <= 4 characters of c, less the first of them while `skip` lasts (the zeros in front of a number)
__device__ __forceinline__ void text_put_skip(TextEmit& E, uint32_t c, uint32_t have, uint32_t& skip) {
  const uint32_t s = skip < have ? skip : have;
  skip -= s;
  E.put(s >= 4u ? 0u : c >> (8u * s), have - s);
}

// y < 10^8: eight characters
__device__ __forceinline__ void text_put8(TextEmit& E, uint32_t y, uint32_t& skip) {
  const uint32_t hi = y / 10000u;
  text_put_skip(E, text_chars4(hi), 4u, skip);
  text_put_skip(E, text_chars4(y - hi * 10000u), 4u, skip);
}

__device__ __forceinline__ void text_put_count(TextEmit& E, uint64_t v) {
  if(!(v >> 32)) {                                                 // 32-bit arithmetic only: ten characters, zeros in front skipped
    const uint32_t x = (uint32_t)v, p1 = x / 100000000u;
    uint32_t skip = 10u - text_digits32(x);
    const uint32_t a = p1 / 10u;
    text_put_skip(E, 0x3030u + (a | ((p1 - a * 10u) << 8)), 2u, skip);
    text_put8(E, x - p1 * 100000000u, skip);
  } else {                                                         // twenty characters: 4 + 8 + 8
    const uint64_t p2 = v / 10000000000000000ull, r = v - p2 * 10000000000000000ull;
    const uint32_t p1 = (uint32_t)(r / 100000000ull), p0 = (uint32_t)(r - (uint64_t)p1 * 100000000ull);
    uint32_t skip = 20u - text_digits(v);
    text_put_skip(E, text_chars4((uint32_t)p2), 4u, skip);
    text_put8(E, p1, skip);
    text_put8(E, p0, skip);
  }
}

// the mer of the record at s_rec: key bytes from the top down, four characters a byte through the table s_tab
// (s_tab[b]: the characters of the bit pairs of b, the highest pair in the low byte)
__device__ __forceinline__ void text_put_mer(TextEmit& E, const uint8_t* s_rec, const uint32_t* s_tab, uint32_t k, uint32_t kb) {
  uint32_t b = kb;
  const uint32_t r = k & 3u;                                       // characters of a partial top byte: its low 2r bits
  if(r) { --b; E.put(s_tab[((uint32_t)s_rec[b] << (8u - 2u * r)) & 0xFFu] & ((1u << (8u * r)) - 1u), r); }
  while(b) { --b; E.put(s_tab[s_rec[b]], 4u); }
}

// out + tile_off[tile] is where the tile's text starts; nothing is written when the text of all tiles (totals[0]) does
// not fit cap_bytes.
__global__ __launch_bounds__(kTextBlock) void text_write_kernel(TextJob J, const uint8_t* __restrict__ raw, uint64_t n, const uint64_t* __restrict__ tile_off,
                                                                const uint64_t* __restrict__ totals, uint64_t cap_bytes, uint8_t* __restrict__ out) {
  JF_DYN_LDS(lds);
  __shared__ uint32_t s_tab[256];
  __shared__ uint32_t s_w[kTextBlock / 64];
  if(totals[0] > cap_bytes) return;
  const uint32_t lane = threadIdx.x;
  {
    const uint32_t acgt = 0x54474341u;                             // "ACGT"
    auto ch = [&](uint32_t c) { return (acgt >> (8u * (c & 3u))) & 0xFFu; };
    s_tab[lane] = ch(lane >> 6) | (ch(lane >> 4) << 8) | (ch(lane >> 2) << 16) | (ch(lane) << 24);
  }
  const uint32_t cnt = text_stage(raw, n, J.rb, (uint4*)lds);      // (its barrier covers s_tab)
  uint8_t* sb = (uint8_t*)lds + text_lds_raw(J.rb);
  uint64_t val;
  const uint32_t len = text_line_len(J, (const uint32_t*)lds, cnt, val);
  // exclusive scan of the lengths: inside the wave by shuffles, across the four waves through LDS
  uint32_t incl = len;
  for(uint32_t o = 1; o < 64u; o <<= 1) { const uint32_t t = __shfl_up(incl, o, 64); if((lane & 63u) >= o) incl += t; }
  if((lane & 63u) == 63u) s_w[lane >> 6] = incl;
  __syncthreads();
  uint32_t off = incl - len, total = 0;
  for(uint32_t w = 0; w < (uint32_t)kTextBlock / 64; ++w) { if(w < (lane >> 6)) off += s_w[w]; total += s_w[w]; }
  const uint64_t gbase = tile_off[blockIdx.x];
  const uint32_t mis = (uint32_t)(((uint64_t)(uintptr_t)out + gbase) & 3u);
  if(len) {
    TextEmit E;
    E.begin(sb, mis + off);
    const uint8_t* s_rec = (const uint8_t*)lds + lane * J.rb;
    if(J.layout == kTextFasta) {
      E.put('>', 1u);
      text_put_count(E, val);
      E.put('\n', 1u);
      text_put_mer(E, s_rec, s_tab, J.k, J.kb);
    } else {
      text_put_mer(E, s_rec, s_tab, J.k, J.kb);
      E.put(J.sep & 0xFFu, 1u);
      text_put_count(E, val);
    }
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
