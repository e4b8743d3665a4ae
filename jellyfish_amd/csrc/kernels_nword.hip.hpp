// jellyfish_amd/csrc/kernels_nword.hip.hpp -- keys of more than two words, 65 <= k <= 128 (gfx950).
//
// The reference's mer_dna is any number of 64-bit words (include/jellyfish/mer_dna.hpp:143-170, 711-717) and its own
// test of the multi-word key path counts 100-mers (tests/large_key.sh:7-18).  Here such keys are 256-bit values in
// four-word slots, the two-word design of kernels_wide.hip.hpp with two more "lo" words:
//
//   slot = { lo0, lo1, lo2, hi }     lo_i = [ tag bits 63i .. 63i+62 | valid ]     hi = [ count | occ | tag >> 189 ]
//
// claim: CAS(hi, 0 -> occ|tag_hi), then CAS(lo_i, 0 -> lo_i) for i = 0, 1, 2: a lane goes on to word i+1 only while
// every word so far equals its own, so the lane that sets the last word matched all the others and the slot holds
// exactly that lane's key; a lane that meets a foreign word probes on, nobody waits (the reference's per-word "set"
// bits, offsets_key_value.hpp:28-31, large_hash_array.hpp:542-579).  Tiles are 2048 slots (64 KiB, what the sorted
// dump sorts in LDS).  Insert paths: the direct kernel here (global atomics), and the partitioned one of
// kernels_nword_part.hip.hpp (P1n, P2, Tn: the same claim on LDS words).
#pragma once
#include "kernels.hip.hpp"
#include "kernels_bloom.hip.hpp"

namespace jfgpu {

constexpr uint32_t kNTileBits = 11;
constexpr uint32_t kNWords = 4;                 // words per key and per slot
constexpr uint32_t kNLoBits = 63 * (kNWords - 1);

struct K256 { uint64_t w[4]; };

JF_HD K256 k256_zero() { K256 r; r.w[0] = r.w[1] = r.w[2] = r.w[3] = 0; return r; }
JF_HD bool k256_eq(const K256& a, const K256& b) { return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3]; }
JF_HD bool k256_less(const K256& a, const K256& b) {      // numeric, from the top word: mer_dna::operator< (mer_dna.hpp:227-250)
  for(int i = 3; i >= 0; --i) if(a.w[i] != b.w[i]) return a.w[i] < b.w[i];
  return false;
}
JF_HD K256 k256_and(const K256& a, const K256& b) { K256 r; for(int i = 0; i < 4; ++i) r.w[i] = a.w[i] & b.w[i]; return r; }
JF_HD K256 k256_or(const K256& a, const K256& b) { K256 r; for(int i = 0; i < 4; ++i) r.w[i] = a.w[i] | b.w[i]; return r; }
JF_HD K256 k256_shr(const K256& a, uint32_t n) {          // n < 256
  const uint32_t ws = n >> 6, bs = n & 63;
  K256 r;
  for(uint32_t i = 0; i < 4; ++i) {
    const uint64_t lo = i + ws < 4 ? a.w[i + ws] : 0, hi = i + ws + 1 < 4 ? a.w[i + ws + 1] : 0;
    r.w[i] = bs ? (lo >> bs) | (hi << (64 - bs)) : lo;
  }
  return r;
}
JF_HD K256 k256_shl(const K256& a, uint32_t n) {          // n < 256
  const uint32_t ws = n >> 6, bs = n & 63;
  K256 r;
  for(int i = 3; i >= 0; --i) {
    const uint64_t hi = i >= (int)ws ? a.w[i - ws] : 0, lo = i >= (int)ws + 1 ? a.w[i - ws - 1] : 0;
    r.w[i] = bs ? (hi << bs) | (lo >> (64 - bs)) : hi;
  }
  return r;
}
JF_HD K256 k256_low_mask(uint32_t bits) {                  // 2^bits - 1, bits <= 256
  K256 r;
  for(uint32_t i = 0; i < 4; ++i) r.w[i] = bits >= 64 * (i + 1) ? ~0ull : (bits > 64 * i ? ((1ull << (bits - 64 * i)) - 1) : 0ull);
  return r;
}
JF_HD K256 k256_from64(uint64_t v) { K256 r = k256_zero(); r.w[0] = v; return r; }
JF_HD uint64_t k256_chunk63(const K256& a, uint32_t i) { return k256_shr(a, 63 * i).w[0] & 0x7FFFFFFFFFFFFFFFull; }

// the rolling updates of mer_iterator (mer_iterator.hpp:67-76): m = (m << 2 | code) & mask, rcm = rcm >> 2 | (3 - code) << 2(k-1)
JF_HD void k256_roll_fw(K256& x, uint64_t c, const K256& mask) {
  x.w[3] = ((x.w[3] << 2) | (x.w[2] >> 62)) & mask.w[3];
  x.w[2] = ((x.w[2] << 2) | (x.w[1] >> 62)) & mask.w[2];
  x.w[1] = ((x.w[1] << 2) | (x.w[0] >> 62)) & mask.w[1];
  x.w[0] = ((x.w[0] << 2) | c) & mask.w[0];
}
JF_HD void k256_roll_rc(K256& x, uint64_t v, uint32_t bitpos) {
  x.w[0] = (x.w[0] >> 2) | (x.w[1] << 62);
  x.w[1] = (x.w[1] >> 2) | (x.w[2] << 62);
  x.w[2] = (x.w[2] >> 2) | (x.w[3] << 62);
  x.w[3] = x.w[3] >> 2;
  x.w[bitpos >> 6] |= v << (bitpos & 63);
}
JF_HD K256 revcomp256(const K256& x, uint32_t k) {
  K256 r;                                                  // reverse all 128 2-bit groups and complement, then drop the padding
  for(int i = 0; i < 4; ++i) r.w[i] = revcomp64(x.w[3 - i], 32);
  return k256_shr(r, 256 - 2 * k);
}

struct NGeom {
  TableGeom g;          // tag_bits / occ_bit / low_mask / inc / cnt_* describe the HI word
  uint32_t tag_full;    // tile_bits + rem_bits
  uint32_t pad_[3];
  K256 key_mask;
};

inline uint32_t nword_min_lsize(uint32_t k) {
  int need = (int)(2 * k + kNTileBits) - (int)kNLoBits - (int)(63 - kMinCountBits);
  if(need < (int)kNTileBits) need = kNTileBits;
  return (uint32_t)need;
}
// shard_bits / shard_id: one shard of a table spread over GPUs, as wide_geom_init (kernels_wide.hip.hpp): the shard owns
// the global positions whose top shard_bits bits are shard_id and holds at least one tile.  The tag is that of the whole
// table (rem_bits = key_bits - lsize_g): the shard id is implied by the rank.
inline bool nword_geom_init(NGeom& N, uint32_t k, uint32_t lsize_g, uint32_t canonical, uint32_t shard_bits = 0, uint32_t shard_id = 0) {
  TableGeom& g = N.g;
  if(k < 65 || k > 128 || lsize_g > 63 || shard_bits > lsize_g || lsize_g - shard_bits < kNTileBits) return false;
  memset(&g, 0, sizeof g);
  g.k = k; g.key_bits = 2 * k; g.lsize_g = lsize_g; g.lsize_l = lsize_g - shard_bits; g.shard_bits = shard_bits; g.shard_id = shard_id;
  g.tile_bits = kNTileBits;
  g.rem_bits = g.key_bits - lsize_g;
  N.tag_full = g.tile_bits + g.rem_bits;
  const uint32_t th = N.tag_full > kNLoBits ? N.tag_full - kNLoBits : 0;
  if(th + 1 + kMinCountBits > 64) return false;
  g.tag_bits = th; g.cnt_bits = 63 - th;
  g.nbytes = (g.key_bits + 7) / 8;
  g.canonical = canonical;
  g.key_mask = ~0ull;
  N.key_mask = k256_low_mask(g.key_bits);
  g.tile_mask = (1ull << g.tile_bits) - 1;
  g.local_mask = (1ull << g.lsize_l) - 1;
  g.occ_bit = 1ull << th;
  g.low_mask = (g.occ_bit << 1) - 1;
  g.inc = g.occ_bit << 1;
  g.cnt_max = (1ull << g.cnt_bits) - 1;
  return true;
}

struct NTable {
  NGeom N;
  uint64_t* slots;            // [4 << lsize]: slot s = slots[4s .. 4s+3] = { lo0, lo1, lo2, hi }
  const uint64_t* fwd_tbl;    // [nbytes * 256]
  const uint64_t* inv_tbl;
  uint64_t* ovf_key; uint64_t* ovf_cnt; uint64_t ovf_mask;
  uint64_t* counters;
  uint32_t max_probe;
  DevBloom bloom;             // count --bc / --bf-size filter (data == nullptr: none)
};

__device__ inline DevTable ovf_view(const NTable& T) {
  DevTable d; d.g = T.N.g; d.slots = nullptr; d.fwd_tbl = nullptr; d.inv_tbl = nullptr;
  d.ovf_key = T.ovf_key; d.ovf_cnt = T.ovf_cnt; d.ovf_mask = T.ovf_mask; d.counters = T.counters; d.max_probe = T.max_probe;
  d.bloom.data = nullptr; d.dirty = nullptr;
  return d;
}

__device__ inline uint64_t hash_tables_n256(const uint64_t* tbl, const K256& key, uint32_t nbytes) {
  uint64_t pos = 0;
  for(uint32_t b = 0; b < nbytes; ++b) pos ^= tbl[b * 256 + ((key.w[b >> 3] >> (8 * (b & 7))) & 0xFF)];
  return pos;
}

// Bloom counter on keys of three and four words: h0 = M1 * key, h1 = M2 * key with 64 x 2k matrices
// (mer_dna_bloom_counter.hpp:19-34); the byte tables (up to 32 x 256 entries each) are read through the caches.
__device__ inline bool bloom_admits_nword(const DevBloom& B, const K256& key) {
  const uint64_t h0 = hash_tables_n256(B.tbl1, key, B.nbytes), h1 = hash_tables_n256(B.tbl2, key, B.nbytes);
  return B.kind == 1 ? bloom_filter_insert(B, h0, h1) : bloom_all_two(B, h0, h1);
}

struct NSlot { uint64_t lo[3]; uint64_t hi_low; };

__device__ inline NSlot nword_tag_words(const NGeom& N, const K256& tag) {      // tag = (idx0 << rem_bits) | (key >> lsize_g)
  NSlot s;
  for(uint32_t i = 0; i < 3; ++i) s.lo[i] = (k256_chunk63(tag, i) << 1) | 1ull;
  s.hi_low = N.g.occ_bit | k256_shr(tag, kNLoBits).w[0];
  return s;
}
__device__ inline NSlot nword_words(const NGeom& N, const K256& key, uint32_t idx0) {
  return nword_tag_words(N, k256_or(k256_shl(k256_from64(idx0), N.g.rem_bits), k256_shr(key, N.g.lsize_g)));
}

__device__ inline K256 nword_slot_key(const NTable& T, const uint64_t* inv_tbl, const uint64_t* slot, uint64_t tile_base) {
  const NGeom& N = T.N;
  K256 tag = k256_shl(k256_from64(slot[3] & (N.g.occ_bit - 1)), kNLoBits);
  for(uint32_t i = 0; i < 3; ++i) tag = k256_or(tag, k256_shl(k256_from64(slot[i] >> 1), 63 * i));
  const K256 rem = k256_and(tag, k256_low_mask(N.g.rem_bits));
  const uint64_t idx0 = k256_shr(tag, N.g.rem_bits).w[0];
  const K256 hi_part = k256_shl(rem, N.g.lsize_g);
  K256 v = hi_part; v.w[0] |= ((uint64_t)N.g.shard_id << N.g.lsize_l) | tile_base | idx0;     // (the shard prefix goes back into the position)
  K256 key = hi_part; key.w[0] |= hash_tables_n256(inv_tbl, v, N.g.nbytes);
  return key;
}

// Where `key` lives, or false when its position names another shard (counted: a key is never silently inserted or
// credited on a shard that does not own it -- jfgpu_sync reports it).
__device__ inline bool nword_addr(const NTable& T, const uint64_t* fwd, const K256& key, SlotAddr& a) {
  a = slot_addr(T.N.g, hash_tables_n256(fwd, key, T.N.g.nbytes));
  if(a.shard == T.N.g.shard_id) return true;
  atomicAdd((unsigned long long*)&T.counters[CTR_MISROUTED], 1ull);
  return false;
}

// claim-or-increment of the slot words `w` in the tile at tile_base, probing from idx0.  Returns true when the key was new
// (this lane set the last word).  The partitioned path's way out of a full region claims with it too (kernels_nword_part.hip.hpp).
template <bool RETURNING>
__device__ inline bool nword_claim(const NTable& T, const NSlot& w, uint64_t tile_base, uint32_t idx0, uint64_t cnt) {
  const TableGeom& g = T.N.g;
  const uint64_t add = cnt << (g.tag_bits + 1);
  for(uint32_t p = 0; p <= T.max_probe; ++p) {
    const uint64_t slot = tile_base + probe_slot(idx0, p, (uint32_t)g.tile_mask);
    unsigned long long* sp = (unsigned long long*)&T.slots[4 * slot];
    const unsigned long long old = atomicCAS(sp + 3, 0ull, (unsigned long long)w.hi_low);
    if(old != 0ull && (old & g.low_mask) != w.hi_low) continue;
    bool mine = true, set_last = false;
    for(uint32_t i = 0; i < 3 && mine; ++i) {
      const unsigned long long l = atomicCAS(sp + i, 0ull, (unsigned long long)w.lo[i]);
      if(l != 0ull && l != w.lo[i]) mine = false;
      else if(i == 2) set_last = l == 0ull;
    }
    if(!mine) continue;
    if(add) {
      if(RETURNING) {
        const unsigned long long prev = atomicAdd(sp + 3, (unsigned long long)add);
        if((prev >> (g.tag_bits + 1)) + cnt > g.cnt_max) { const DevTable d = ovf_view(T); ovf_add(d, slot, 1); }
      } else {
        __hip_atomic_fetch_add(sp + 3, (unsigned long long)add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    return set_last;
  }
  atomicAdd((unsigned long long*)&T.counters[CTR_FULL], 1ull);
  return false;
}

// claim-or-increment at the key's home.
template <bool RETURNING>
__device__ inline bool nword_add_at(const NTable& T, const K256& key, const SlotAddr& a, uint64_t cnt) {
  return nword_claim<RETURNING>(T, nword_words(T.N, key, a.idx0), a.tile_base, a.idx0, cnt);
}

template <bool RETURNING>
__device__ inline bool nword_add(const NTable& T, const K256& key, uint64_t cnt) {
  SlotAddr a;
  return nword_addr(T, T.fwd_tbl, key, a) && nword_add_at<RETURNING>(T, key, a, cnt);
}

// Slot holding `key` in the tile of `a`, or ~0 when it is absent (a look-up: the first never-claimed slot ends the search).
__device__ inline uint64_t nword_find_at(const NTable& T, const K256& key, const SlotAddr& a) {
  const TableGeom& g = T.N.g;
  const NSlot w = nword_words(T.N, key, a.idx0);
  for(uint32_t p = 0; p <= T.max_probe; ++p) {
    const uint64_t slot = a.tile_base + probe_slot(a.idx0, p, (uint32_t)g.tile_mask);
    const uint64_t* sp = &T.slots[4 * slot];
    const uint64_t hi = __hip_atomic_load(sp + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if(hi == 0) return ~0ull;
    if((hi & g.low_mask) != w.hi_low) continue;
    if(__hip_atomic_load(sp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == w.lo[0] &&
       __hip_atomic_load(sp + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == w.lo[1] &&
       __hip_atomic_load(sp + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == w.lo[2]) return slot;
  }
  return ~0ull;
}
__device__ inline uint64_t nword_find(const NTable& T, const uint64_t* fwd, const K256& key) {     // (a key of another shard is not here)
  const SlotAddr a = slot_addr(T.N.g, hash_tables_n256(fwd, key, T.N.g.nbytes));
  return a.shard == T.N.g.shard_id ? nword_find_at(T, key, a) : ~0ull;
}

__device__ inline void nword_credit(const NTable& T, uint64_t slot, uint64_t cnt) {    // add to an existing slot
  const TableGeom& g = T.N.g;
  const unsigned long long prev = atomicAdd((unsigned long long*)&T.slots[4 * slot + 3], (unsigned long long)(cnt << (g.tag_bits + 1)));
  if((prev >> (g.tag_bits + 1)) + cnt > g.cnt_max) { const DevTable d = ovf_view(T); ovf_add(d, slot, 1); }
}

// hash_counter::add(key, val) with any 64-bit val
__device__ inline bool nword_add_val(const NTable& T, const uint64_t* fwd, const K256& key, uint64_t val) {
  const TableGeom& g = T.N.g;
  const uint64_t lowpart = val & g.cnt_max, units = val >> g.cnt_bits;
  SlotAddr a;
  if(!nword_addr(T, fwd, key, a)) return false;
  const bool is_new = nword_add_at<true>(T, key, a, lowpart);
  if(units) { const uint64_t s = nword_find_at(T, key, a); if(s != ~0ull) { const DevTable d = ovf_view(T); ovf_add(d, s, units); } }
  return is_new;
}

// update_add: increment only if the key is there (the UPDATE pass of `count --if`); the add always reads the old count back
__device__ inline bool nword_update_add(const NTable& T, const uint64_t* fwd, const K256& key, uint64_t cnt) {
  SlotAddr a;
  if(!nword_addr(T, fwd, key, a)) return false;
  const uint64_t s = nword_find_at(T, key, a);
  if(s != ~0ull) nword_credit(T, s, cnt);
  return s != ~0ull;
}

__device__ inline uint64_t nword_count_at(const NTable& T, const DevTable& d, uint64_t slot, uint64_t hi, int have_ovf) {
  uint64_t c = slot_count(T.N.g, hi);
  if(have_ovf) c += ovf_get(d, slot) << T.N.g.cnt_bits;
  return c;
}
__device__ inline bool nword_complete(const uint64_t* sp) { return sp[3] != 0 && sp[0] != 0 && sp[1] != 0 && sp[2] != 0; }

// ---- sequence -> 256-bit k-mers -----------------------------------------------------------------------------
// Halo: k - 1 <= 127 bases = 8 code words before the lane's own 16.  Validity is tracked the way mer_iterator does
// (`filled`): the number of consecutive valid bases ending at the current position, capped at k.
// FILTERED: count --bc / --bf-size (count_main.cc:115-131) -- T.bloom is asked for every valid sighting, before the run
// merge (a one-pass filter changes as it is asked: once per run would undercount); CTR_MERS counts every window either way.
template <bool RETURNING, bool FILTERED>
__global__ __launch_bounds__(kBlock) void count_ascii_nword_kernel(NTable T, const uint8_t* __restrict__ base, int64_t lo, int64_t hi, int op) {
  __shared__ uint32_t s_codes[kBlock + 8];
  __shared__ uint32_t s_inv[kBlock + 8];
  __shared__ int s_abort;
  const NGeom& N = T.N;
  const uint32_t k = N.g.k, rc_pos = 2 * (k - 1);
  const int tid = threadIdx.x;
  const int64_t n_tiles = (hi + kTilePos - 1) / kTilePos;
  uint32_t my_mers = 0;
  for(int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    if(tid == 0) s_abort = __hip_atomic_load(&T.counters[CTR_FULL], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
    __syncthreads();
    if(s_abort) break;
    const int64_t tile_start = tile * kTilePos;
    uint32_t c, v;
    load_pack16(base, tile_start + 16 * tid, lo, hi, c, v);
    s_codes[tid + 8] = c; s_inv[tid + 8] = v;
    if(tid < 8) { uint32_t hc, hv; load_pack16(base, tile_start - 128 + 16 * tid, lo, hi, hc, hv); s_codes[tid] = hc; s_inv[tid] = hv; }
    __syncthreads();
    // the k-mer ending just before this lane (garbage where bases were invalid: `filled` guards it)
    K256 fw;
    for(int i = 0; i < 4; ++i) fw.w[i] = ((uint64_t)s_codes[tid + 7 - 2 * i - 1] << 32) | s_codes[tid + 7 - 2 * i];
    fw = k256_and(fw, N.key_mask);
    K256 rc = revcomp256(fw, k);
    uint32_t filled = 0;
    for(int q = 7; q >= 0; --q) {                          // nearest halo word first
      const uint32_t iv = s_inv[tid + q] & 0xFFFFu;
      if(iv == 0) { filled += 16; continue; }
      filled += (uint32_t)__ffs((int)iv) - 1;              // valid bases after the word's last invalid one
      break;
    }
    if(filled > k) filled = k;
    K256 prev = k256_zero(); uint32_t run = 0;
    auto apply = [&](const K256& key, uint32_t n) {
      if(op == 0) nword_add<RETURNING>(T, key, n);
      else if(op == 1) nword_add<RETURNING>(T, key, 0);
      else { const uint64_t s = nword_find(T, T.fwd_tbl, key); if(s != ~0ull) nword_credit(T, s, n); }
    };
#pragma unroll 1
    for(int j = 0; j < kPerLane; ++j) {
      const uint64_t code = (c >> (2 * (15 - j))) & 3u;
      k256_roll_fw(fw, code, N.key_mask);
      k256_roll_rc(rc, 3ull - code, rc_pos);
      if((v >> (15 - j)) & 1u) { filled = 0; continue; }
      if(filled < k) ++filled;
      if(filled < k) continue;
      ++my_mers;
      const K256 key = (N.g.canonical && k256_less(rc, fw)) ? rc : fw;
      if constexpr(FILTERED) { if(!bloom_admits_nword(T.bloom, key)) continue; }
      if(run && k256_eq(key, prev)) { ++run; continue; }
      if(run) apply(prev, run);
      prev = key; run = 1;
    }
    if(run) apply(prev, run);
  }
  uint64_t w = my_mers;
  for(int o = 32; o > 0; o >>= 1) w += __shfl_down(w, o, 64);
  if((threadIdx.x & 63) == 0 && w) atomicAdd((unsigned long long*)&T.counters[CTR_MERS], (unsigned long long)w);
}

// keys come as ceil(2k / 64) words each (3 for k <= 96), the reference's mer_dna::data() layout
__device__ inline K256 load_key4(const uint64_t* keys, uint64_t i, uint32_t kw, const K256& mask) {
  K256 r = k256_zero();
  for(uint32_t q = 0; q < kw; ++q) r.w[q] = keys[(uint64_t)kw * i + q];
  return k256_and(r, mask);
}

// ---- sequence -> 256-bit k-mers for the routing kernels (route_count / route_scatter_kernel, kernels.hip.hpp) --------------
// The buffer is read like count_ascii_nword_kernel reads it (halo of 8 code words, `filled` validity, canonical form).  The
// matrix's byte tables (up to 32 x 256 words, 64 KiB) sit in dynamic LDS there: a k-mer's 32 gathers go to LDS, not to L2.
// Per-owner counts never become an atomic per k-mer: the lanes of a wave that route to the same owner are grouped by ballot
// (one LDS atomic per wave and owner, and consecutive ranks in lane order), so a wave's k-mers for one owner land in
// neighbouring records.
struct NLane { uint32_t c, v, filled; K256 fw, rc; };     // a lane's 16 bases and the k-mer state just before them

// f(j, key, valid) for the lane's 16 positions, called by every lane at every position (wave-uniform: f may ballot)
template <typename F>
__device__ inline void for_each_kmer_nword(const NGeom& N, NLane L, F&& f) {
  const uint32_t k = N.g.k, rc_pos = 2 * (k - 1);
#pragma unroll                                             // (unrolled: the callers' per-position arrays stay in registers)
  for(int j = 0; j < kPerLane; ++j) {
    const uint64_t code = (L.c >> (2 * (15 - j))) & 3u;
    k256_roll_fw(L.fw, code, N.key_mask);
    k256_roll_rc(L.rc, 3ull - code, rc_pos);
    if((L.v >> (15 - j)) & 1u) L.filled = 0;
    else if(L.filled < k) ++L.filled;
    f(j, (N.g.canonical && k256_less(L.rc, L.fw)) ? L.rc : L.fw, L.filled >= k && !((L.v >> (15 - j)) & 1u));
  }
}

// The rank of this lane's k-mer among the workgroup's k-mers of owner s (s_hist[s] grows by one LDS atomic per wave and
// owner).  Called by every lane of the wave; valid: this lane has a k-mer here.
__device__ inline uint32_t nword_wave_rank(bool valid, uint32_t s, uint32_t* s_hist) {
  const uint32_t lane = threadIdx.x & 63;
  uint64_t pending = __ballot(valid);
  uint32_t rank = 0;
  while(pending) {                                         // (wave-uniform: one round per distinct owner in the wave)
    const int leader = __ffsll((long long)pending) - 1;
    const uint32_t so = __shfl(s, leader, 64);
    const bool mine = valid && s == so;
    const uint64_t m = __ballot(mine);
    uint32_t b = 0;
    if((int)lane == leader) b = atomicAdd(&s_hist[so], (uint32_t)__popcll(m));
    b = __shfl(b, leader, 64);
    if(mine) rank = b + (uint32_t)__popcll(m & ((1ull << lane) - 1));
    pending &= ~m;
  }
  return rank;
}

// Slot access for the kernels written once for every key width (KeyOps, kernels.hip.hpp).  A slot is looked at where it lies (in
// the table, or in the dump's copy of it); only a complete one -- every word set -- holds a key, whatever the kernel.
template <> struct KeyOps<NTable> {
  typedef K256 Key;
  struct Slot { const uint64_t* sp; };
  static constexpr int kSlotWords = kNWords;
  static constexpr uint32_t kFwdLdsWords = 0;            // up to 32 x 256 words = 64 KiB: read through the caches
  static constexpr bool kUpdateReturns = true;
  typedef NLane Lane;
  static constexpr uint32_t kHaloWords = 8, kKeyWords = 0;   // (3 or 4 words a key: the caller's kw)
  __device__ static const TableGeom& geom(const NTable& T) { return T.N.g; }
  __device__ static bool load(const NTable& T, uint64_t i, Slot& s) { s.sp = &T.slots[4 * i]; return nword_complete(s.sp); }
  __device__ static bool occupied(const NTable& T, uint64_t i, Slot& s) { return load(T, i, s); }
  __device__ static Slot slot_of(const uint64_t* w) { Slot s; s.sp = w; return s; }
  __device__ static uint64_t count(const NTable& T, const Slot& s, uint64_t i, int have_ovf) { return nword_count_at(T, ovf_view(T), i, s.sp[3], have_ovf); }
  __device__ static Key key(const NTable& T, const Slot& s, uint64_t tile_base) { return nword_slot_key(T, T.inv_tbl, s.sp, tile_base); }
  __device__ static uint64_t count_at(const NTable& T, uint64_t i, int have_ovf) { return nword_count_at(T, ovf_view(T), i, T.slots[4 * i + 3], have_ovf); }
  __device__ static const uint64_t* stage_fwd(const NTable& T) { return T.fwd_tbl; }
  __device__ static bool add_val(const NTable& T, const uint64_t* H, const Key& key, uint64_t val) { return nword_add_val(T, H, key, val); }
  template <bool RETURNING>
  __device__ static bool update_add(const NTable& T, const uint64_t* H, const Key& key, uint64_t cnt) { static_assert(RETURNING, "kUpdateReturns"); return nword_update_add(T, H, key, cnt); }
  __device__ static uint64_t find(const NTable& T, const uint64_t* H, const Key& key) { return nword_find(T, H, key); }
  __device__ static uint32_t owner(const NTable& T, const uint64_t* H, const Key& key) { return slot_addr(T.N.g, hash_tables_n256(H, key, T.N.g.nbytes)).shard; }
  __device__ static void store_key(uint64_t* dst, const Key& key, uint32_t kw) { for(uint32_t q = 0; q < kw; ++q) dst[q] = key.w[q]; }
  __device__ static Key load_key(const NTable& T, const uint64_t* keys, uint64_t i, uint32_t kw, bool) { return load_key4(keys, i, kw, T.N.key_mask); }   // (masked either way)
  __device__ static uint64_t digest(const NTable& T, const Key& key, uint64_t c) {
    uint64_t h = kDigestSeed;
    for(uint32_t q = 0; q < (T.N.g.k + 31) / 32; ++q) h = digest_mix(h ^ key.w[q]);
    return digest_mix(h ^ c);
  }
  __device__ static uint8_t key_byte(const Key& key, uint32_t b) { return (uint8_t)(key.w[b >> 3] >> (8 * (b & 7))); }
  // (the staging itself and not a call of it: the Lane handed back through one more function costs route_count_kernel two
  // VGPRs, profiles/route_kernel_resources.txt)
  __device__ static Lane stage_tile(const NTable& T, const uint8_t* __restrict__ base, int64_t tile_start, int64_t lo, int64_t hi, uint32_t* s_codes, uint32_t* s_inv) {
    const NGeom& N = T.N;
    const int tid = threadIdx.x;
    NLane L;
    load_pack16(base, tile_start + 16 * tid, lo, hi, L.c, L.v);
    s_codes[tid + 8] = L.c; s_inv[tid + 8] = L.v;
    if(tid < 8) { uint32_t hc, hv; load_pack16(base, tile_start - 128 + 16 * tid, lo, hi, hc, hv); s_codes[tid] = hc; s_inv[tid] = hv; }
    __syncthreads();
    for(int i = 0; i < 4; ++i) L.fw.w[i] = ((uint64_t)s_codes[tid + 7 - 2 * i - 1] << 32) | s_codes[tid + 7 - 2 * i];
    L.fw = k256_and(L.fw, N.key_mask);
    L.rc = revcomp256(L.fw, N.g.k);
    L.filled = 0;
    for(int q = 7; q >= 0; --q) {                            // nearest halo word first
      const uint32_t iv = s_inv[tid + q] & 0xFFFFu;
      if(iv == 0) { L.filled += 16; continue; }
      L.filled += (uint32_t)__ffs((int)iv) - 1;
      break;
    }
    if(L.filled > N.g.k) L.filled = N.g.k;
    return L;
  }
  template <typename F>
  __device__ static void for_each_kmer(const NTable& T, const Lane& L, F&& f) { for_each_kmer_nword(T.N, L, f); }
  __device__ static bool same_key(const Key& a, const Key& b) { return k256_eq(a, b); }
  __device__ static Key text_key(const NTable& T, const Lane& L, int j) {      // (L.fw: the k-mer ending just before the lane)
    Key r = k256_shl(L.fw, 2 * j + 2);
    r.w[0] |= L.c >> (30 - 2 * j);
    return k256_and(r, T.N.key_mask);
  }
  __device__ static uint32_t route_rank(bool valid, uint32_t owner, uint32_t* s_hist) { return nword_wave_rank(valid, owner, s_hist); }
};

// ---- Bloom counter over keys of three and four words (jellyfish bc, 65 <= k <= 128) ---------------------------------------
// Every valid window is one bloom_insert (no run merge: a k-mer seen twice in a row must read 2).  The two byte tables
// (2 x ceil(2k / 8) x 2 KiB: 100 KiB at k = 100, 128 KiB at k = 128) are read through the caches, as the two-word kernel
// reads its 64 KiB and count_ascii_nword_kernel its own (DESIGN.md 3.5 on staging them in LDS instead).
__global__ __launch_bounds__(kBlock) void bloom_insert_ascii_nword_kernel(DevBloom B, NGeom N, const uint8_t* __restrict__ base,
                                                                          int64_t lo, int64_t hi, unsigned long long* __restrict__ mers) {
  __shared__ uint32_t s_codes[kBlock + 8];
  __shared__ uint32_t s_inv[kBlock + 8];
  NTable T; T.N = N;                                       // (stage_tile and for_each_kmer look at the geometry only)
  const int64_t n_tiles = (hi + kTilePos - 1) / kTilePos;
  uint32_t my = 0;
  for(int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    __syncthreads();
    const NLane L = KeyOps<NTable>::stage_tile(T, base, tile * kTilePos, lo, hi, s_codes, s_inv);
    for_each_kmer_nword(N, L, [&](int, const K256& key, bool valid) {
      if(!valid) return;
      ++my;
      bloom_insert(B, hash_tables_n256(B.tbl1, key, B.nbytes), hash_tables_n256(B.tbl2, key, B.nbytes));
    });
  }
  uint64_t w = my;
  for(int o = 32; o > 0; o >>= 1) w += __shfl_down(w, o, 64);
  if((threadIdx.x & 63) == 0 && w) atomicAdd(mers, (unsigned long long)w);
}

// check() / insert() on encoded keys of kw = ceil(2k / 64) words each (mer_dna::data() layout)
__global__ __launch_bounds__(kBlock) void bloom_keys_nword_kernel(DevBloom B, K256 key_mask, uint32_t kw, const uint64_t* __restrict__ keys, uint64_t n,
                                                                  uint8_t* __restrict__ out, int do_insert) {
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const K256 key = load_key4(keys, i, kw, key_mask);
    const uint64_t h0 = hash_tables_n256(B.tbl1, key, B.nbytes), h1 = hash_tables_n256(B.tbl2, key, B.nbytes);
    const uint32_t r = do_insert ? bloom_insert(B, h0, h1) : bloom_check(B, h0, h1);
    if(out) out[i] = (uint8_t)r;
  }
}

}  // namespace jfgpu
