// jellyfish_amd/csrc/kernels_bgzf.hip.hpp -- BGZF inflate and BAM record decode, on the device (gfx950).
//
// SURVEY row 14 (`count --sam`): the reference reads SAM / BAM through htslib (include/jellyfish/sam_format.hpp,
// mer_overlap_sequence_parser.hpp:220-250), one record at a time on a CPU thread.  Here the compressed bytes cross PCIe
// and everything after the member headers runs on the device:
//
//   A  bgzf_inflate_kernel   one wave per BGZF block (<= 64 KiB in, <= 64 KiB out): a complete RFC 1951 inflate (stored,
//                            fixed and dynamic Huffman blocks), output staged in LDS, ISIZE and CRC32 checked, then the
//                            block is written coalesced at its offset in the inflated stream
//   B  bam_guess_kernel      per 64 KiB segment of the inflated stream: the first offset that looks like a record start
//                            (plausibility checks), then the record chain from there to the segment's end
//   C  bam_fix_kernel        one workgroup: the chain from the known first record, segment to segment -- a segment whose
//                            guessed entry is not its predecessor's exit is walked again from the true entry (rounds until
//                            nothing changes) -- then exclusive scans of records and output bytes per segment
//   D  bam_list_kernel       per segment: the verified chain, record starts and output offsets
//   E  bam_emit_kernel       one wave per record: 4-bit bases -> ACGT / N, quality mask, the 'N' separator
//
// The inflate is written for the whole wave to run the same decode: every lane reads the same bits and the same table
// entries (LDS broadcasts, one cache line), so there is no divergence; the LZ77 copies are split across the lanes, each
// byte taken from out[pos - dist + (i mod dist)] (a source always written before the copy started), and literals are
// stored by lane 0.  Correctness of B-D does not depend on the guesses: C rebuilds the chain wherever they are wrong.
#pragma once
#include "kernels.hip.hpp"

namespace jfgpu {

// ---------------------------------------------------------------- inflate
constexpr int kInfLut = 10;                            // bits of the first-level Huffman lookup
constexpr int kInfOut = 65536;                         // a BGZF block inflates to at most 64 KiB
// dynamic LDS layout of bgzf_inflate_kernel (bytes)
constexpr int kInfOffCrc = kInfOut;                    // 256 x u32 CRC32 table
constexpr int kInfOffLitLut = kInfOffCrc + 1024;       // 1024 x u16: symbol | length << 9 (0: slow path)
constexpr int kInfOffDistLut = kInfOffLitLut + 2048;
constexpr int kInfOffLitCnt = kInfOffDistLut + 2048;   // 16 x u16 codes per length
constexpr int kInfOffDistCnt = kInfOffLitCnt + 32;
constexpr int kInfOffOffs = kInfOffDistCnt + 32;       // 16 x u16 scratch of the table build
constexpr int kInfOffLitSym = kInfOffOffs + 32;        // 288 x u16 symbols in canonical order
constexpr int kInfOffDistSym = kInfOffLitSym + 576;    // 32 x u16
constexpr int kInfOffLens = kInfOffDistSym + 64;       // 320 x u8 code lengths
constexpr int kInfOffFlag = kInfOffLens + 320;         // u32: table build failed
constexpr int kInfLds = kInfOffFlag + 16;              // 71,776 bytes: two waves per CU

__device__ __forceinline__ uint64_t bz_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

__constant__ uint8_t kInfOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};   // RFC 1951 3.2.7

enum : uint32_t {
  INF_OK = 0, INF_BAD_TYPE = 1, INF_BAD_STORED = 2, INF_BAD_TABLE = 3, INF_BAD_CODE = 4, INF_BAD_DIST = 5,
  INF_OVERFLOW = 6, INF_OVERRUN = 7, INF_BAD_ISIZE = 8, INF_BAD_CRC = 9
};

__device__ __forceinline__ uint32_t crc_mulmod(uint32_t a, uint32_t b) {   // a(x) b(x) mod P(x), reflected bit order
  uint32_t p = 0;
  for(int i = 0; i < 32; ++i) {
    if(a & (0x80000000u >> i)) p ^= b;
    b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
  }
  return p;
}
// x^(8 n) mod P: what n zero bytes do to a CRC register
__device__ __forceinline__ uint32_t crc_shift_bytes(uint32_t n) {
  uint32_t r = 0x80000000u, sq = 0x00800000u;          // x^0, x^8
  for(; n; n >>= 1) {
    if(n & 1) r = crc_mulmod(r, sq);
    sq = crc_mulmod(sq, sq);
  }
  return r;
}

struct InfBits {
  const uint8_t* src;   // 4-byte aligned base of the compressed buffer
  uint64_t bb;          // bit buffer, next bit in bit 0
  int bc;               // valid bits in bb
  uint64_t ip;          // next 4-byte word to load (byte offset, multiple of 4)
  uint64_t lim;         // loads at or past this offset mean the block ran past its end
};
__device__ __forceinline__ void inf_seek(InfBits& s, uint64_t byte) {
  s.ip = byte & ~(uint64_t)3;
  const uint32_t w = *(const uint32_t*)(s.src + s.ip);
  const int sh = (int)(byte & 3) * 8;
  s.bb = (uint64_t)(w >> sh); s.bc = 32 - sh; s.ip += 4;
}
__device__ __forceinline__ bool inf_refill(InfBits& s) {       // >= 32 bits in bb afterwards; false: past the block
  if(s.bc >= 32) return true;
  if(s.ip >= s.lim) return false;
  s.bb |= (uint64_t)(*(const uint32_t*)(s.src + s.ip)) << s.bc;
  s.ip += 4; s.bc += 32;
  return true;
}
__device__ __forceinline__ uint32_t inf_bits(InfBits& s, int n) {   // n <= 32, refilled before
  const uint32_t v = (uint32_t)(s.bb & ((1ull << n) - 1));
  s.bb >>= n; s.bc -= n;
  return v;
}

// Canonical Huffman tables from lens[0..n): counts, symbols in code order, and the first-level lookup (codes of at most
// kInfLut bits; longer ones read bit by bit from cnt / sym).  Over-subscribed sets fail.  Incomplete sets fail as they
// do in zlib (inftrees.c), so that the verdict on a stream is the reference reader's: the code-length code must be
// complete (INF_SET_COMPLETE); a literal / length or distance set may be incomplete only when it has no code longer
// than one bit, that is a single code of length 1 or no code at all (INF_SET_DYNAMIC); the fixed distance code, 30 of
// 32 codes, is kept as it is (INF_SET_ANY).  An unassigned code of a set that was kept fails to decode.  Every lane
// calls it; lane 0 does the serial part.
enum : int { INF_SET_COMPLETE = 0, INF_SET_DYNAMIC = 1, INF_SET_ANY = 2 };
__device__ void inf_build(uint8_t* lds, const uint8_t* lens, int n, int rule, uint16_t* cnt, uint16_t* sym, uint16_t* lut, unsigned lane) {
  uint16_t* offs = (uint16_t*)(lds + kInfOffOffs);
  uint32_t* flag = (uint32_t*)(lds + kInfOffFlag);
  __syncthreads();                                             // every lane is done with the previous tables
  for(int i = lane; i < (1 << kInfLut); i += 64) lut[i] = 0;
  if(lane == 0) {
    for(int l = 0; l < 16; ++l) cnt[l] = 0;
    for(int s = 0; s < n; ++s) cnt[lens[s]]++;
    cnt[0] = 0;
    int left = 1, bad = 0, longest = 0;
    for(int l = 1; l < 16 && !bad; ++l) { left <<= 1; left -= cnt[l]; if(left < 0) bad = 1; if(cnt[l]) longest = l; }
    if(left > 0 && (rule == INF_SET_COMPLETE || (rule == INF_SET_DYNAMIC && longest > 1))) bad = 1;
    offs[1] = 0;
    for(int l = 1; l < 15; ++l) offs[l + 1] = offs[l] + cnt[l];
    for(int s = 0; s < n; ++s) if(lens[s]) sym[offs[lens[s]]++] = (uint16_t)s;
    *flag = bad;
  }
  __syncthreads();
  if(*flag) return;
  // symbol i of the code order: its length and code (codes of one length are consecutive)
  int total = 0;
  for(int l = 1; l < 16; ++l) total += cnt[l];
  for(int i = lane; i < total; i += 64) {
    int l = 1, first = 0, idx = 0, code = 0;
    for(; l < 16; ++l) {
      if(i < idx + cnt[l]) { code = first + (i - idx); break; }
      idx += cnt[l]; first = (first + cnt[l]) << 1;
    }
    if(l > kInfLut) continue;
    uint32_t r = 0;
    for(int b = 0; b < l; ++b) r |= ((code >> b) & 1u) << (l - 1 - b);     // the stream sends codes MSB first
    const uint16_t e = (uint16_t)(sym[i] | (l << 9));
    for(uint32_t f = r; f < (1u << kInfLut); f += (1u << l)) lut[f] = e;
  }
  __syncthreads();
}

// one symbol; bb holds >= 15 bits.  -1: no such code
__device__ __forceinline__ int inf_decode(InfBits& s, const uint16_t* cnt, const uint16_t* sym, const uint16_t* lut) {
  const uint16_t e = lut[s.bb & ((1u << kInfLut) - 1)];
  if(e) { const int l = e >> 9; s.bb >>= l; s.bc -= l; return e & 511; }
  int code = 0, first = 0, idx = 0;
  for(int l = 1; l < 16; ++l) {
    code |= (int)(s.bb & 1); s.bb >>= 1; s.bc -= 1;
    const int c = cnt[l];
    if(code - first < c) return sym[idx + code - first];
    idx += c; first = (first + c) << 1; code <<= 1;
  }
  return -1;
}

// grid: one 64-thread workgroup per block; dynamic LDS kInfLds.  d_comp: 4-byte aligned, readable 16 bytes past every
// block's deflate data.  d_err: min over failing blocks of (block << 8 | INF_*), ~0 when all are good.
__global__ __launch_bounds__(64) void bgzf_inflate_kernel(const uint8_t* __restrict__ d_comp, const jfgpu_bgzf_block* __restrict__ blocks,
                                                          uint8_t* __restrict__ d_dst, unsigned long long* d_err) {
  JF_DYN_LDS(lds);
  const unsigned lane = threadIdx.x;
  const uint64_t blk = blockIdx.x;
  const jfgpu_bgzf_block B = blocks[blk];
  uint8_t* out = lds;
  uint32_t* crc_tab = (uint32_t*)(lds + kInfOffCrc);
  uint16_t* lit_lut = (uint16_t*)(lds + kInfOffLitLut);
  uint16_t* dist_lut = (uint16_t*)(lds + kInfOffDistLut);
  uint16_t* lit_cnt = (uint16_t*)(lds + kInfOffLitCnt);
  uint16_t* dist_cnt = (uint16_t*)(lds + kInfOffDistCnt);
  uint16_t* lit_sym = (uint16_t*)(lds + kInfOffLitSym);
  uint16_t* dist_sym = (uint16_t*)(lds + kInfOffDistSym);
  uint8_t* lens = lds + kInfOffLens;
  uint32_t* flag = (uint32_t*)(lds + kInfOffFlag);
  for(uint32_t i = lane; i < 256; i += 64) {
    uint32_t c = i;
    for(int b = 0; b < 8; ++b) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    crc_tab[i] = c;
  }
  InfBits s;
  s.src = d_comp; s.lim = B.c_off + B.c_len + 8;
  inf_seek(s, B.c_off);
  const uint32_t isize = B.isize;
  uint32_t op = 0, err = INF_OK, last = 0;
  while(!last && !err) {
    if(!inf_refill(s)) { err = INF_OVERRUN; break; }
    last = inf_bits(s, 1);
    const uint32_t type = inf_bits(s, 2);
    if(type == 0) {                                              // stored
      inf_bits(s, s.bc & 7);                                     // to a byte boundary
      if(!inf_refill(s)) { err = INF_OVERRUN; break; }
      const uint32_t len = inf_bits(s, 16), nlen = inf_bits(s, 16);
      if(len != (~nlen & 0xFFFFu)) { err = INF_BAD_STORED; break; }
      const uint64_t at = s.ip - (uint64_t)(s.bc >> 3);          // byte offset of the first stored byte
      if(at + len > (uint64_t)B.c_off + B.c_len) { err = INF_OVERRUN; break; }
      if(op + len > isize) { err = INF_OVERFLOW; break; }
      for(uint32_t i = lane; i < len; i += 64) out[op + i] = d_comp[at + i];
      op += len;
      inf_seek(s, at + len);
      __syncthreads();
      continue;
    }
    if(type == 3) { err = INF_BAD_TYPE; break; }
    if(type == 1) {                                              // fixed Huffman codes
      if(lane == 0) {
        for(int i = 0; i < 144; ++i) lens[i] = 8;
        for(int i = 144; i < 256; ++i) lens[i] = 9;
        for(int i = 256; i < 280; ++i) lens[i] = 7;
        for(int i = 280; i < 288; ++i) lens[i] = 8;
        for(int i = 0; i < 30; ++i) lens[288 + i] = 5;
      }
      __syncthreads();
      inf_build(lds, lens, 288, INF_SET_COMPLETE, lit_cnt, lit_sym, lit_lut, lane);
      inf_build(lds, lens + 288, 30, INF_SET_ANY, dist_cnt, dist_sym, dist_lut, lane);
    } else {                                                     // dynamic: the code-length code, then the two codes
      const uint32_t nlen = inf_bits(s, 5) + 257, ndist = inf_bits(s, 5) + 1, ncode = inf_bits(s, 4) + 4;
      if(nlen > 286 || ndist > 30) { err = INF_BAD_TABLE; break; }
      if(!inf_refill(s)) { err = INF_OVERRUN; break; }
      __syncthreads();                                           // nobody reads lens any more
      if(lane == 0) for(int i = 0; i < 19; ++i) lens[i] = 0;
      for(uint32_t i0 = 0; i0 < ncode; i0 += 10) {              // 3 bits each, at most 10 per refill
        if(!inf_refill(s)) { err = INF_OVERRUN; break; }
        const uint32_t m = bz_min(ncode - i0, 10u);
        if(lane == 0) for(uint32_t i = 0; i < m; ++i) lens[kInfOrder[i0 + i]] = (uint8_t)((s.bb >> (3 * i)) & 7);
        inf_bits(s, (int)(3 * m));
      }
      __syncthreads();
      if(err) break;
      inf_build(lds, lens, 19, INF_SET_COMPLETE, lit_cnt, lit_sym, lit_lut, lane);
      if(*flag) { err = INF_BAD_TABLE; break; }
      // literal / length lengths go to lens[0..nlen), distance lengths to lens[288..288+ndist)
      uint32_t idx = 0, prev = 0;                                 // prev: the last length written, by whichever symbol
      while(idx < nlen + ndist) {
        if(!inf_refill(s)) { err = INF_OVERRUN; break; }
        const int sym = inf_decode(s, lit_cnt, lit_sym, lit_lut);
        if(sym < 0) { err = INF_BAD_CODE; break; }
        uint32_t v, rep;
        if(sym < 16) { v = (uint32_t)sym; rep = 1; prev = v; }
        else if(sym == 16) { if(idx == 0) { err = INF_BAD_TABLE; break; } v = prev; rep = 3 + inf_bits(s, 2); }
        else if(sym == 17) { v = 0; rep = 3 + inf_bits(s, 3); prev = 0; }
        else { v = 0; rep = 11 + inf_bits(s, 7); prev = 0; }
        if(idx + rep > nlen + ndist) { err = INF_BAD_TABLE; break; }
        if(lane == 0) for(uint32_t r = 0; r < rep; ++r) { const uint32_t i = idx + r; lens[i < nlen ? i : 288 + i - nlen] = (uint8_t)v; }
        idx += rep;
      }
      if(err) break;
      __syncthreads();
      if(lens[256] == 0) { err = INF_BAD_TABLE; break; }         // no end-of-block code
      inf_build(lds, lens, (int)nlen, INF_SET_DYNAMIC, lit_cnt, lit_sym, lit_lut, lane);
      if(*flag) { err = INF_BAD_TABLE; break; }
      inf_build(lds, lens + 288, (int)ndist, INF_SET_DYNAMIC, dist_cnt, dist_sym, dist_lut, lane);
    }
    if(*flag) { err = INF_BAD_TABLE; break; }
    for(;;) {                                                    // the codes of one block
      if(!inf_refill(s)) { err = INF_OVERRUN; break; }
      const int sym = inf_decode(s, lit_cnt, lit_sym, lit_lut);
      if(sym < 0) { err = INF_BAD_CODE; break; }
      if(sym < 256) {
        if(op >= isize) { err = INF_OVERFLOW; break; }
        if(lane == 0) out[op] = (uint8_t)sym;
        ++op;
        continue;
      }
      if(sym == 256) break;
      const uint32_t ls = (uint32_t)sym - 257;
      if(ls >= 29) { err = INF_BAD_CODE; break; }
      uint32_t len;
      if(ls < 8) len = 3 + ls;
      else if(ls == 28) len = 258;
      else { const uint32_t eb = (ls - 4) >> 2; len = ((4 + (ls & 3)) << eb) + 3 + inf_bits(s, (int)eb); }
      if(!inf_refill(s)) { err = INF_OVERRUN; break; }
      const int ds = inf_decode(s, dist_cnt, dist_sym, dist_lut);
      if(ds < 0 || ds >= 30) { err = INF_BAD_CODE; break; }
      uint32_t dist;
      if(ds < 4) dist = (uint32_t)ds + 1;
      else { const uint32_t eb = ((uint32_t)ds >> 1) - 1; dist = ((2 + ((uint32_t)ds & 1)) << eb) + 1 + inf_bits(s, (int)eb); }
      if(dist > op) { err = INF_BAD_DIST; break; }
      if(op + len > isize) { err = INF_OVERFLOW; break; }
      __syncthreads();                                           // every byte before op is in LDS
      const uint32_t from = op - dist;
      if(dist >= len) { for(uint32_t i = lane; i < len; i += 64) out[op + i] = out[from + i]; }
      else { for(uint32_t i = lane; i < len; i += 64) out[op + i] = out[from + i % dist]; }
      op += len;
    }
  }
  __syncthreads();
  if(!err && op != isize) err = INF_BAD_ISIZE;
  if(!err && (s.ip - (uint64_t)(s.bc >> 3)) > (uint64_t)B.c_off + B.c_len) err = INF_OVERRUN;   // the last bit used lies inside the data
  if(!err) {
    // CRC32: lane j takes bytes [j*seg, (j+1)*seg), its register moved past the bytes behind them, xor over the wave
    const uint32_t seg = (isize + 63) / 64;
    const uint32_t a = bz_min(isize, lane * seg), b = bz_min(isize, a + seg);
    uint32_t c = lane == 0 ? 0xFFFFFFFFu : 0u;
    for(uint32_t i = a; i < b; ++i) c = crc_tab[(c ^ out[i]) & 255] ^ (c >> 8);
    c = crc_mulmod(c, crc_shift_bytes(isize - b));
    for(int o = 32; o > 0; o >>= 1) c ^= __shfl_xor(c, o, 64);
    if((~c) != B.crc32) err = INF_BAD_CRC;
  }
  if(err) {
    if(lane == 0) atomicMin(d_err, (unsigned long long)(blk << 8 | err));
    return;
  }
  uint8_t* dst = d_dst + B.u_off;
  for(uint32_t i = lane; i < isize; i += 64) dst[i] = out[i];
}

// ---------------------------------------------------------------- BAM records
constexpr uint32_t kBamSeg = 65536;                    // bytes of inflated stream per segment
constexpr uint64_t kBamNone = ~0ull;

__device__ __forceinline__ uint32_t bam_u16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ int32_t bam_i32(const uint8_t* p) {
  return (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
}

struct BamWalk { uint64_t exit; uint64_t out; uint32_t recs; uint32_t bad; };

// The record chain from p while records start before end.  Stops at a record that is not complete in [0, n) (it is
// carried to the next chunk); bad = a record whose lengths do not add up (a corrupt stream, or a wrong guess).
__device__ BamWalk bam_walk(const uint8_t* S, uint64_t n, uint64_t p, uint64_t end) {
  BamWalk w = {p, 0, 0, 0};
  while(p < end) {
    if(p + 4 > n) break;
    const int32_t bs = bam_i32(S + p);
    if(bs < 32) { w.bad = 1; break; }
    if(p + 4 + (uint64_t)bs > n) break;
    const uint32_t l_name = S[p + 12], n_cig = bam_u16(S + p + 16);
    const int32_t l_seq = bam_i32(S + p + 20);
    if(l_name < 1 || l_seq < 0 || 32ull + l_name + 4ull * n_cig + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq > (uint64_t)bs) { w.bad = 1; break; }
    w.recs++; w.out += (uint64_t)l_seq + 1;
    p += 4 + (uint64_t)bs;
  }
  w.exit = p;
  return w;
}

// Does a complete, self-consistent record start at q?  (Only a guess: bam_fix_kernel checks it.)
__device__ bool bam_plausible(const uint8_t* S, uint64_t n, uint64_t q, int32_t n_ref) {
  if(q + 36 > n) return false;
  const int32_t bs = bam_i32(S + q);
  if(bs < 33 || q + 4 + (uint64_t)bs > n) return false;
  const int32_t ref = bam_i32(S + q + 4), pos = bam_i32(S + q + 8), nref = bam_i32(S + q + 24), npos = bam_i32(S + q + 28);
  if(ref < -1 || ref >= n_ref || nref < -1 || nref >= n_ref || pos < -1 || npos < -1) return false;
  const uint32_t l_name = S[q + 12], n_cig = bam_u16(S + q + 16);
  const int32_t l_seq = bam_i32(S + q + 20);
  if(l_name < 1 || l_seq < 0 || 32ull + l_name + 4ull * n_cig + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq > (uint64_t)bs) return false;
  const uint8_t* name = S + q + 36;
  if(name[l_name - 1] != 0) return false;
  for(uint32_t i = 0; i + 1 < l_name; ++i) if(name[i] < '!' || name[i] > '~') return false;
  return true;
}

struct BamSeg { uint64_t entry, exit, out; uint32_t recs, bad; };

__global__ __launch_bounds__(256) void bam_guess_kernel(const uint8_t* __restrict__ S, uint64_t n, uint64_t f0, uint32_t nseg, int32_t n_ref,
                                                        BamSeg* __restrict__ seg) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if(s >= nseg) return;
  const uint64_t a = f0 + (uint64_t)s * kBamSeg, b = bz_min(n, a + kBamSeg);
  uint64_t g = s == 0 ? f0 : kBamNone;
  if(s) for(uint64_t q = a; q < b; ++q) if(bam_plausible(S, n, q, n_ref)) { g = q; break; }
  BamSeg r = {g, kBamNone, 0, 0, 0};
  if(g != kBamNone) { const BamWalk w = bam_walk(S, n, g, b); r.exit = w.exit; r.out = w.out; r.recs = w.recs; r.bad = w.bad; }
  seg[s] = r;
}

struct BamTotals { uint64_t recs, out, end; uint32_t bad, rounds; };

// One workgroup of 1024: rounds of "entry := predecessor's exit, walk again where that changed the entry", then the
// exclusive scans.  rec_off / out_off get the scans, tot the totals and the end of the last complete record.
__global__ __launch_bounds__(1024) void bam_fix_kernel(const uint8_t* __restrict__ S, uint64_t n, uint64_t f0, uint32_t nseg, BamSeg* seg,
                                                       uint64_t* want, uint64_t* rec_off, uint64_t* out_off, BamTotals* tot) {
  __shared__ uint32_t s_changed;
  __shared__ uint64_t s_r[1024], s_o[1024];
  __shared__ uint32_t s_bad;
  const uint32_t t = threadIdx.x;
  uint32_t rounds = 0;
  for(;;) {
    if(t == 0) s_changed = 0;
    for(uint32_t s = t; s < nseg; s += 1024) want[s] = s == 0 ? f0 : seg[s - 1].exit;
    __syncthreads();
    uint32_t ch = 0;
    for(uint32_t s = t; s < nseg; s += 1024) {
      const uint64_t w = want[s];
      if(w == kBamNone) { ch = 1; continue; }                    // the predecessor has no chain yet
      if(w == seg[s].entry) continue;
      const uint64_t b = bz_min(n, f0 + (uint64_t)(s + 1) * kBamSeg);
      const BamWalk r = bam_walk(S, n, w, b);
      BamSeg v = {w, r.exit, r.out, r.recs, r.bad};
      seg[s] = v;
      ch = 1;
    }
    if(ch) atomicOr(&s_changed, 1u);
    __syncthreads();
    ++rounds;
    const uint32_t c = s_changed;
    __syncthreads();
    if(!c || rounds > nseg + 2) break;
  }
  // exclusive scans over segments: thread t sums a contiguous range, a scan over the threads, then the range again
  const uint32_t per = (nseg + 1023) / 1024, a = bz_min(nseg, t * per), b = bz_min(nseg, a + per);
  uint64_t r = 0, o = 0; uint32_t bad = 0;
  for(uint32_t s = a; s < b; ++s) { r += seg[s].recs; o += seg[s].out; bad |= seg[s].bad; }
  if(t == 0) s_bad = 0;
  s_r[t] = r; s_o[t] = o;
  __syncthreads();
  if(bad) atomicOr(&s_bad, 1u);
  for(uint32_t d = 1; d < 1024; d <<= 1) {
    const uint64_t pr = t >= d ? s_r[t - d] : 0, po = t >= d ? s_o[t - d] : 0;
    __syncthreads();
    s_r[t] += pr; s_o[t] += po;
    __syncthreads();
  }
  r = s_r[t] - r; o = s_o[t] - o;                              // exclusive
  for(uint32_t s = a; s < b; ++s) { rec_off[s] = r; out_off[s] = o; r += seg[s].recs; o += seg[s].out; }
  if(t == 1023) {
    BamTotals v;
    v.recs = s_r[1023]; v.out = s_o[1023]; v.end = nseg ? seg[nseg - 1].exit : f0;
    v.bad = s_bad | (rounds > nseg + 2 ? 2u : 0u); v.rounds = rounds;
    *tot = v;
  }
}

__global__ __launch_bounds__(256) void bam_list_kernel(const uint8_t* __restrict__ S, uint64_t n, uint64_t f0, uint32_t nseg, const BamSeg* __restrict__ seg,
                                                       const uint64_t* __restrict__ rec_off, const uint64_t* __restrict__ out_off,
                                                       uint64_t* __restrict__ rec_start, uint64_t* __restrict__ rec_out) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if(s >= nseg) return;
  const uint64_t b = bz_min(n, f0 + (uint64_t)(s + 1) * kBamSeg);
  uint64_t p = seg[s].entry, r = rec_off[s], o = out_off[s];
  for(uint32_t i = 0; i < seg[s].recs && p < b; ++i) {         // the chain bam_fix_kernel verified
    rec_start[r] = p; rec_out[r] = o;
    o += (uint64_t)bam_i32(S + p + 20) + 1;
    p += 4 + (uint64_t)bam_i32(S + p);
    ++r;
  }
}

// One wave per record: the 4-bit bases (1 A, 2 C, 4 G, 8 T, anything else N: sam_format.hpp decode), a base whose
// quality character (char)(q + '!') is below min_qual (signed compare, mer_qual_iterator.hpp:76-77) becomes N, then
// the separator.
__global__ __launch_bounds__(256) void bam_emit_kernel(const uint8_t* __restrict__ S, uint64_t nrec, const uint64_t* __restrict__ rec_start,
                                                       const uint64_t* __restrict__ rec_out, uint32_t min_qual, uint8_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64);
  for(uint64_t r = (uint64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; r < nrec; r += waves) {
    const uint64_t p = rec_start[r];
    const uint32_t l_name = S[p + 12], n_cig = bam_u16(S + p + 16);
    const uint32_t l_seq = (uint32_t)bam_i32(S + p + 20);
    const uint8_t* seq = S + p + 36 + l_name + 4ull * n_cig;
    const uint8_t* qual = seq + (l_seq + 1) / 2;
    uint8_t* o = out + rec_out[r];
    for(uint32_t i = lane; i < l_seq; i += 64) {
      const uint32_t nib = (i & 1) ? (seq[i >> 1] & 15u) : (uint32_t)(seq[i >> 1] >> 4);
      uint8_t c = nib == 1 ? 'A' : nib == 2 ? 'C' : nib == 4 ? 'G' : nib == 8 ? 'T' : 'N';
      if(min_qual && (int)(int8_t)(uint8_t)(qual[i] + 33) < (int)min_qual) c = 'N';
      o[i] = c;
    }
    if(lane == 0) o[l_seq] = 'N';
  }
}

}  // namespace jfgpu
