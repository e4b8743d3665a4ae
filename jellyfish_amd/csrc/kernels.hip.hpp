// jellyfish_amd/csrc/kernels.hip.hpp -- gfx950 (CDNA4) device code of the hot path.
//
// What each kernel replaces in the reference (paths relative to /root/reference):
//   count_ascii_kernel   the COUNT loop of mer_counter_base::start
//                        (sub_commands/count_main.cc:152-163): mer_iterator
//                        (mer_iterator.hpp:53-81) + RectangularBinaryMatrix::times
//                        (rectangular_binary_matrix.hpp:155-164) + array_base::add
//                        (large_hash_array.hpp:291-295,509-597,741-752)
//   add_keys_kernel      hash_counter::add on encoded mers (hash_counter.hpp:91-126)
//   lookup_kernel        array_base::get_val_for_key (large_hash_array.hpp:354-372)
//   route_*_kernel       new: hash-prefix routing of k-mers to their owning GPU
//   stats/histo/dump     region iterators + sorted_dumper + binary_writer
//                        (large_hash_iterator.hpp, sorted_dumper.hpp:57-101,
//                        binary_dumper.hpp:36-40)
//
// Design notes (see DESIGN.md for the numbers):
//   * wave64 everywhere; blocks of 256 threads = 4 waves, one per SIMD.
//   * sequence bytes are read once, 16 B per lane (1 KiB per wave-instruction),
//     converted to 2-bit codes + an invalid mask in registers and exchanged with
//     the neighbouring lanes through LDS (k-1 <= 31 bases of halo = two words).
//   * the GF(2) hash is 2k/8 LDS table look-ups (the matrix is linear), not
//     2k select-XORs.
//   * the table lives in HBM as 64-bit slots; claim = one 64-bit atomicCAS,
//     increment = one 64-bit atomicAdd.  Integer / indexing work: no MFMA.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kmer_core.hpp"

namespace jfgpu {

constexpr int kBlock = 256;
constexpr int kPerThread = kPerLane;           // positions per lane per tile (16)
constexpr int kTilePos = kBlock * kPerThread;  // 4096 sequence positions per block iteration

enum Counter : int { CTR_FULL = 0, CTR_MERS = 1, CTR_OVF_FULL = 2, CTR_OVF_USED = 3, CTR_MISROUTED = 4, CTR_DIRECT = 5,
                     CTR_T_ITEMS = 6, CTR_T_QUEUED = 7 /* tile stage: items placed / items past rank 3 (the sampling launch of a flush) */,
                     CTR_PROF0 = 8 /* .. 11: phase clocks of a -DJFGPU_TILE_PROF build */, CTR_COUNT = 12 };

// -DJFGPU_PHASE_PROF builds: shader clocks per phase of the partition kernels, as wave 0 of every block sees them,
// summed over blocks into a device array the host prints at jfgpu_sync (tools/build_libs.sh builds it, JFGPU_LIB selects it).  Slots 0-7 P1, 8-15 P2, 16-23 T.
#ifdef JFGPU_PHASE_PROF
__device__ unsigned long long g_phase_prof[24];
struct PhaseClk {
  long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}; long long t;
  __device__ PhaseClk() { t = clock64(); }
  __device__ void mark(int i) { const long long n = clock64(); acc[i] += n - t; t = n; }
  __device__ void flush(int base) { if(threadIdx.x == 0) for(int i = 0; i < 8; ++i) if(acc[i]) atomicAdd(&g_phase_prof[base + i], (unsigned long long)acc[i]); }
};
#define JF_PHASE(pc, i) (pc).mark(i)
#define JF_PHASE_FLUSH(pc, base) (pc).flush(base)
#else
struct PhaseClk {};
#define JF_PHASE(pc, i) do {} while(0)
#define JF_PHASE_FLUSH(pc, base) do {} while(0)
#endif

// Bloom counter view (kernels_bloom.hip.hpp); data == nullptr: no filter attached.
struct DevBloom {
  uint32_t* data;             // ceil(m/5) bytes, addressed as dwords
  uint64_t m;                 // number of base-3 cells
  uint64_t recip;             // floor(2^64 / m): x % m without a 64-bit divide (the reference's divisor64, divisor.hpp:64-109)
  uint32_t nh;                // hash functions per key
  uint32_t nbytes;            // key bytes fed to the tables
  uint32_t kind;              // 0: Bloom counter, admit iff check() > 1 (count --bc); 1: one-pass Bloom filter, insert and admit iff
  uint32_t pad_;              //    every bit was already set (count --bf-size, count_main.cc:121-131)
  const uint64_t* tbl1;       // byte tables of the two 64-row matrices
  const uint64_t* tbl2;
  // count --bc on high-coverage input: k-mers the counter has ADMITTED before (bloom_admit_mask), two-way sets of
  // key + 1 (0: empty); nullptr: off.  A hit answers for the ten cell reads; only admitted keys are ever stored, and an
  // admitted key stays admitted (the cells saturate), so the answers are the counter's own (kernels_bloom.hip.hpp)
  uint64_t* cache;
  uint64_t cache_mask;        // sets - 1
};

struct DevTable {
  TableGeom g;
  uint64_t* slots;            // [1 << lsize_l]
  const uint64_t* fwd_tbl;    // [nbytes * 256]   key -> pos
  const uint64_t* inv_tbl;    // [nbytes * 256]   (rem, pos) -> low key bits
  uint64_t* ovf_key;          // overflow side table, keyed by slot index + 1 (0 = empty)
  uint64_t* ovf_cnt;          // units of 2^cnt_bits
  uint64_t ovf_mask;          // capacity - 1
  uint64_t* counters;         // [CTR_COUNT]
  uint32_t max_probe;         // last probe index tried before declaring the tile full
  DevBloom bloom;             // count --bc filter (data == nullptr: none)
  uint8_t* dirty;             // one byte per tile: something was ever inserted (tile_insert may skip reading clean tiles)
};

// Workgroup barrier that orders LDS only.  __syncthreads() also waits for every outstanding
// global store of the wave (s_waitcnt vmcnt(0)), which serialises "write a chunk to HBM" with
// "start the next chunk" in the streaming kernels; here the only cross-wave traffic is LDS.
// (JFGPU_EMU: the same sources compiled for the host by tests/host/hip_emu, where a barrier is a fiber rendezvous.)
#if defined(JFGPU_EMU)
__device__ __forceinline__ void lds_barrier() { __syncthreads(); }
#define JF_DYN_LDS(name) unsigned char* name = ::hip_emu::dyn_lds()
#else
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
#define JF_DYN_LDS(name) extern __shared__ __align__(16) unsigned char name[]
#endif

__device__ inline bool bloom_admits(const DevBloom& B, uint64_t key);   // kernels_bloom.hip.hpp
__device__ inline uint32_t bloom_admit_mask(const DevBloom& B, const TableGeom& g, const LaneWords& L);   // kernels_bloom.hip.hpp

// ---- overflow side table ----------------------------------------------------
// A slot's count field wrapped: remember `units` x 2^cnt_bits for that slot.  Keyed by
// the slot index, which identifies the key (keys never move while the table lives).
__device__ inline void ovf_add(const DevTable& T, uint64_t slot, uint64_t units) {
  const uint64_t want = slot + 1;
  uint64_t h = (slot * 0x9E3779B97F4A7C15ull) >> 20;
  for(uint64_t p = 0; p <= T.ovf_mask; ++p) {
    const uint64_t s = (h + p) & T.ovf_mask;
    unsigned long long old = atomicCAS((unsigned long long*)&T.ovf_key[s], 0ull, (unsigned long long)want);
    if(old == 0ull) atomicAdd((unsigned long long*)&T.counters[CTR_OVF_USED], 1ull);
    if(old == 0ull || old == want) {
      atomicAdd((unsigned long long*)&T.ovf_cnt[s], (unsigned long long)units);
      return;
    }
  }
  atomicAdd((unsigned long long*)&T.counters[CTR_OVF_FULL], 1ull);
}

__device__ inline uint64_t ovf_get(const DevTable& T, uint64_t slot) {
  const uint64_t want = slot + 1;
  uint64_t h = (slot * 0x9E3779B97F4A7C15ull) >> 20;
  for(uint64_t p = 0; p <= T.ovf_mask; ++p) {
    const uint64_t s = (h + p) & T.ovf_mask;
    const uint64_t k = T.ovf_key[s];
    if(k == 0) return 0;
    if(k == want) return T.ovf_cnt[s];
  }
  return 0;
}

__device__ inline uint64_t full_count(const DevTable& T, uint64_t word, uint64_t slot, bool have_ovf) {
  uint64_t c = slot_count(T.g, word);
  if(have_ovf) c += ovf_get(T, slot) << T.g.cnt_bits;
  return c;
}

// ---- slot access ------------------------------------------------------------------
// 64-bit slots, or 32-bit slots holding the same [count | occ | tag] fields (TableGeom::slot32).  The branch is
// uniform over the whole grid (a scalar branch); slot words travel as uint64_t either way.
__device__ __forceinline__ uint64_t slot_ld(const DevTable& T, uint64_t i) {
  return T.g.slot32 ? (uint64_t)reinterpret_cast<const uint32_t*>(T.slots)[i] : T.slots[i];
}
__device__ __forceinline__ uint64_t slot_ld_relaxed(const DevTable& T, uint64_t i) {
  if(T.g.slot32) return __hip_atomic_load(reinterpret_cast<const uint32_t*>(T.slots) + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __hip_atomic_load(&T.slots[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t slot_cas(const DevTable& T, uint64_t i, uint64_t cmp, uint64_t val) {
  if(T.g.slot32) return atomicCAS(reinterpret_cast<unsigned int*>(T.slots) + i, (unsigned int)cmp, (unsigned int)val);
  return atomicCAS((unsigned long long*)&T.slots[i], (unsigned long long)cmp, (unsigned long long)val);
}
__device__ __forceinline__ uint64_t slot_add_rtn(const DevTable& T, uint64_t i, uint64_t add) {
  if(T.g.slot32) return atomicAdd(reinterpret_cast<unsigned int*>(T.slots) + i, (unsigned int)add);
  return atomicAdd((unsigned long long*)&T.slots[i], (unsigned long long)add);
}
__device__ __forceinline__ void slot_add(const DevTable& T, uint64_t i, uint64_t add) {
  if(T.g.slot32) __hip_atomic_fetch_add(reinterpret_cast<unsigned int*>(T.slots) + i, (unsigned int)add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else __hip_atomic_fetch_add((unsigned long long*)&T.slots[i], (unsigned long long)add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- insert / increment -------------------------------------------------------
// large_hash_array.hpp:509-597 (claim_key) + :741-752 (add_val), restated for a
// 64-bit [count|occ|tag] slot: CAS the whole word from 0 to claim, atomicAdd on
// the top field to increment.  Returns true when the key was new.
// RETURNING selects the add that reads back the old value (needed only when the
// count field can wrap; a fire-and-forget add otherwise).
template <bool RETURNING>
__device__ inline bool table_add(const DevTable& T, const uint64_t* fwd_lds, uint64_t key, uint64_t cnt) {
  const TableGeom& g = T.g;
  const uint64_t pos = hash_tables(fwd_lds, key, g.nbytes);
  const SlotAddr a = slot_addr(g, pos);
  if(a.shard != g.shard_id) {  // a key that belongs to another GPU's shard must never land here
    atomicAdd((unsigned long long*)&T.counters[CTR_MISROUTED], 1ull);
    return false;
  }
  { uint8_t* d = &T.dirty[a.tile_base >> g.tile_bits]; if(!*d) *d = 1; }
  const uint64_t tag = make_tag(g, key, a.idx0);
  const uint64_t low = g.occ_bit | tag;
  const uint64_t add = cnt << (g.tag_bits + 1);
  const uint64_t neww = add | low;
  const uint32_t tmask = (uint32_t)g.tile_mask;
  for(uint32_t p = 0; p <= T.max_probe; ++p) {
    const uint64_t slot = a.tile_base + probe_lin(a.idx0, p, tmask);
    const uint64_t old = slot_cas(T, slot, 0, neww);
    if(old == 0ull) return true;
    if((old & g.low_mask) == low) {
      if(RETURNING) {
        const uint64_t prev = slot_add_rtn(T, slot, add);
        if((prev >> (g.tag_bits + 1)) + cnt > g.cnt_max) ovf_add(T, slot, 1);
      } else {
        slot_add(T, slot, add);
      }
      return false;
    }
  }
  atomicAdd((unsigned long long*)&T.counters[CTR_FULL], 1ull);  // tile exhausted: "Hash full"
  return false;
}

// Slot holding `key` in the tile of `a`, or ~0 when it is absent.  Probes like a look-up: the first empty slot ends the search.
__device__ inline uint64_t table_find_at(const DevTable& T, uint64_t key, const SlotAddr& a) {
  const TableGeom& g = T.g;
  const uint64_t low = g.occ_bit | make_tag(g, key, a.idx0);
  const uint32_t tmask = (uint32_t)g.tile_mask;
  for(uint32_t p = 0; p <= T.max_probe; ++p) {
    const uint64_t slot = a.tile_base + probe_lin(a.idx0, p, tmask);
    const uint64_t old = slot_ld_relaxed(T, slot);
    if(old == 0ull) return ~0ull;
    if((old & g.low_mask) == low) return slot;
  }
  return ~0ull;
}

// hash_counter::update_add (hash_counter.hpp:150-166, large_hash_array.hpp update_add): increment only
// if the key is already there -- the UPDATE pass of `count --if` (count_main.cc:173-181).  The probe of table_find_at,
// written out with the add inside the loop: on top of table_find_at the compiler gives count_ascii_kernel, which inlines
// this sixteen times, another register allocation (profiles/keyed_kernel_resources.txt).
template <bool RETURNING>
__device__ inline bool table_update_add(const DevTable& T, const uint64_t* fwd_lds, uint64_t key, uint64_t cnt) {
  const TableGeom& g = T.g;
  const uint64_t pos = hash_tables(fwd_lds, key, g.nbytes);
  const SlotAddr a = slot_addr(g, pos);
  if(a.shard != g.shard_id) { atomicAdd((unsigned long long*)&T.counters[CTR_MISROUTED], 1ull); return false; }
  const uint64_t low = g.occ_bit | make_tag(g, key, a.idx0);
  const uint64_t add = cnt << (g.tag_bits + 1);
  const uint32_t tmask = (uint32_t)g.tile_mask;
  for(uint32_t p = 0; p <= T.max_probe; ++p) {
    const uint64_t slot = a.tile_base + probe_lin(a.idx0, p, tmask);
    const uint64_t old = slot_ld_relaxed(T, slot);
    if(old == 0ull) return false;
    if((old & g.low_mask) == low) {
      if(RETURNING) {
        const uint64_t prev = slot_add_rtn(T, slot, add);
        if((prev >> (g.tag_bits + 1)) + cnt > g.cnt_max) ovf_add(T, slot, 1);
      } else {
        slot_add(T, slot, add);
      }
      return true;
    }
  }
  return false;
}

// Arbitrary 64-bit increment (hash_counter::add(key, val)): split into field-sized pieces.
__device__ inline bool table_add_val(const DevTable& T, const uint64_t* fwd_lds, uint64_t key, uint64_t val) {
  const TableGeom& g = T.g;
  const uint64_t lowpart = val & g.cnt_max;
  const uint64_t units = g.cnt_bits >= 64 ? 0 : (val >> g.cnt_bits);
  // one claim-or-find with the low part (possibly 0: still claims the key, like set())
  const uint64_t pos = hash_tables(fwd_lds, key, g.nbytes);
  const SlotAddr a = slot_addr(g, pos);
  if(a.shard != g.shard_id) {
    atomicAdd((unsigned long long*)&T.counters[CTR_MISROUTED], 1ull);
    return false;
  }
  { uint8_t* d = &T.dirty[a.tile_base >> g.tile_bits]; if(!*d) *d = 1; }
  const uint64_t tag = make_tag(g, key, a.idx0);
  const uint64_t low = g.occ_bit | tag;
  const uint64_t add = lowpart << (g.tag_bits + 1);
  const uint32_t tmask = (uint32_t)g.tile_mask;
  for(uint32_t p = 0; p <= T.max_probe; ++p) {
    const uint64_t slot = a.tile_base + probe_lin(a.idx0, p, tmask);
    const uint64_t old = slot_cas(T, slot, 0, add | low);
    bool mine = false, is_new = false;
    if(old == 0ull) { mine = true; is_new = true; }
    else if((old & g.low_mask) == low) {
      mine = true;
      if(add) {
        const uint64_t prev = slot_add_rtn(T, slot, add);
        if((prev >> (g.tag_bits + 1)) + lowpart > g.cnt_max) ovf_add(T, slot, 1);
      }
    }
    if(mine) {
      if(units) ovf_add(T, slot, units);
      return is_new;
    }
  }
  atomicAdd((unsigned long long*)&T.counters[CTR_FULL], 1ull);
  return false;
}

// ---- slot access per key width ------------------------------------------------------
// What a kernel needs from its view (DevTable here, WideTable in kernels_wide.hip.hpp, NTable in kernels_nword.hip.hpp), so
// that it is written once.  The kernels that walk a whole table: rehash_kernel, scan_kernel and dump_tiles_words_kernel
// below, reshard_kernel and add_pairs_kernel in kernels_comm.hip.hpp.  The kernels that are handed a list of keys: add_keys_kernel,
// update_keys_kernel and lookup_kernel below.  A specialisation has
//   Key, Slot                        a key, and what was read of a slot
//   geom(T)                          the table's TableGeom
//   load(T, i, s)                    reads slot i; true when it holds a key
//   occupied(T, i, s)                the cheaper read where one word tells (the multi-word views; the counting scans use it)
//   count(T, s, i, have_ovf)         the full count, with the overflow side table when have_ovf
//   count_at(T, i, have_ovf)         the same of the slot at index i, read here
//   key(T, s, tile_base)             the key, rebuilt through inv_tbl
//   kFwdLdsWords, stage_fwd(T)       how the forward hash tables reach a keyed kernel: the 64-bit words of static LDS they are
//                                    staged in (0: NTable's 64 KiB stay in global memory, read through the caches), and the
//                                    staging with its barrier, which returns the pointer H the hash is to read.  The
//                                    whole-table kernels hash rarely and pass T.fwd_tbl
//   add_val(T, H, key, val)          hash_counter::add(key, val) into T
//   update_add<RETURNING>(T, H, key, cnt)  hash_counter::update_add: only if the key is there; kUpdateReturns: the view's
//                                    update_add reads the old count back whatever RETURNING says (only <true> is to be compiled)
//   find(T, H, key)                  the slot that holds key, or ~0; a key of another shard is not here
//   owner(T, H, key)                 the shard that owns key under T's matrix
//   store_key / load_key             a key as kw little-endian 64-bit words; load_key masks with the table's key mask when asked
//   digest(T, key, c)                (the multi-word views) an entry's digest hash
//   kSlotWords, slot_of(w), key_byte (the multi-word views, for the dump) words per slot, a slot from a copy of its words, byte b of a key
// and, for the kernels that read sequence from a contract buffer (route_count_kernel and route_scatter_kernel below):
//   Lane, kHaloWords                 a lane's 16 bases with the k-mer state before them, and the code words of halo a tile is
//                                    staged with (k - 1 bases: 2, 4 or 8)
//   stage_tile(T, base, tile_start, lo, hi, s_codes, s_inv)   the tile's codes and invalid masks through LDS (kBlock +
//                                    kHaloWords words each) into a Lane; ends in a barrier
//   for_each_kmer(T, L, f)           f(j, key, valid) for the (canonical) k-mer ending at position j of the lane.  The one- and
//                                    two-word views call f for the valid windows only; NTable calls it on every lane at every
//                                    position (wave-uniform), because its route_rank ballots
//   route_rank(valid, owner, s_hist) the rank of this lane's k-mer among the workgroup's k-mers of its owner, counted in
//                                    s_hist.  One LDS atomic per k-mer for one and two words, one per wave and owner (by
//                                    ballot) for NTable: each width keeps the ranking it was written and measured with, and
//                                    moving the narrow widths to the ballot would be a change of speed, not of structure
//   admit_mask(T, L), admits(T, mask, j, key)   count --bc, only in a BLOOM kernel: what the view's Bloom counter admits.  One
//                                    word asks for the lane's 16 windows at once and tests a bit, two words ask key by key
//                                    (the mask is all ones); NTable takes no filter and has neither
//   kKeyWords                        64-bit words a routed key is stored as by store_key (0: the caller's kw, 3 or 4)
// and, for query_ascii_kernel:
//   same_key(a, b)                   are two keys equal
//   text_key(T, L, j)                the k-mer ending at position j of the lane as the text has it, not its canonical form
//   Probe, find_begin, find_end      (one word) find in two halves, so that a lane's look-ups overlap
template <class Table> struct KeyOps;

__device__ inline void load_tables_lds(uint64_t* dst, const uint64_t* src, uint32_t nbytes) {
  for(uint32_t i = threadIdx.x; i < nbytes * 256; i += blockDim.x) dst[i] = src[i];
}
template <uint32_t WORDS>
__device__ inline const uint64_t* stage_tables_lds(const uint64_t* src, uint32_t nbytes) {     // (KeyOps::stage_fwd of the views that stage)
  __shared__ uint64_t s_tbl[WORDS];
  load_tables_lds(s_tbl, src, nbytes);
  __syncthreads();
  return s_tbl;
}

__device__ inline LaneWords stage_tile(const uint8_t* __restrict__ base, int64_t tile_start, int64_t lo, int64_t hi, uint32_t* s_codes, uint32_t* s_inv);   // below

template <> struct KeyOps<DevTable> {
  typedef uint64_t Key;
  struct Slot { uint64_t w; };
  static constexpr uint32_t kFwdLdsWords = 8 * 256;
  static constexpr bool kUpdateReturns = false;
  typedef LaneWords Lane;
  static constexpr uint32_t kHaloWords = 2, kKeyWords = 1;
  __device__ static const TableGeom& geom(const DevTable& T) { return T.g; }
  __device__ static bool load(const DevTable& T, uint64_t i, Slot& s) { s.w = slot_ld(T, i); return s.w != 0; }
  __device__ static uint64_t count(const DevTable& T, const Slot& s, uint64_t i, int have_ovf) { return full_count(T, s.w, i, have_ovf); }
  __device__ static uint64_t count_at(const DevTable& T, uint64_t i, int have_ovf) { return full_count(T, slot_ld(T, i), i, have_ovf); }
  __device__ static Key key(const DevTable& T, const Slot& s, uint64_t tile_base) { return slot_key(T.g, T.inv_tbl, s.w, tile_base); }
  __device__ static const uint64_t* stage_fwd(const DevTable& T) { return stage_tables_lds<kFwdLdsWords>(T.fwd_tbl, T.g.nbytes); }
  __device__ static bool add_val(const DevTable& T, const uint64_t* H, Key key, uint64_t val) { return table_add_val(T, H, key, val); }
  template <bool RETURNING>
  __device__ static bool update_add(const DevTable& T, const uint64_t* H, Key key, uint64_t cnt) { return table_update_add<RETURNING>(T, H, key, cnt); }
  __device__ static uint64_t find(const DevTable& T, const uint64_t* H, Key key) {
    const SlotAddr a = slot_addr(T.g, hash_tables(H, key, T.g.nbytes));
    return a.shard == T.g.shard_id ? table_find_at(T, key, a) : ~0ull;
  }
  // find in two halves (query_ascii_kernel): find_begin hashes and issues the load of the first slot probed, find_end
  // resolves it and probes on.  Between the two a lane may begin more look-ups, so their line fills overlap.  find_end
  // leaves the word of the slot it returns in p.w.
  struct Probe { uint64_t low, slot, w; };
  __device__ static Probe find_begin(const DevTable& T, const uint64_t* H, Key key) {
    const SlotAddr a = slot_addr(T.g, hash_tables(H, key, T.g.nbytes));
    Probe p;
    p.low = T.g.occ_bit | make_tag(T.g, key, a.idx0);
    p.slot = a.tile_base + probe_lin(a.idx0, 0, (uint32_t)T.g.tile_mask);
    p.w = a.shard == T.g.shard_id ? slot_ld_relaxed(T, p.slot) : 0ull;      // (a key of another shard is not here)
    return p;
  }
  __device__ static uint64_t find_end(const DevTable& T, Probe& p) {
    uint64_t slot = p.slot;
    for(uint32_t q = 0; p.w != 0ull; p.w = slot_ld_relaxed(T, slot)) {
      if((p.w & T.g.low_mask) == p.low) return slot;
      if(++q > T.max_probe) break;
      slot = (p.slot & ~T.g.tile_mask) | ((p.slot + q) & T.g.tile_mask);      // probe_lin: linear from the bucket's start, inside the tile
    }
    return ~0ull;
  }
  __device__ static uint32_t owner(const DevTable& T, const uint64_t* H, Key key) { return (uint32_t)(hash_tables(H, key, T.g.nbytes) >> T.g.lsize_l); }
  __device__ static bool same_key(Key a, Key b) { return a == b; }
  __device__ static void store_key(uint64_t* dst, Key key, uint32_t) { dst[0] = key; }
  __device__ static Key load_key(const DevTable& T, const uint64_t* keys, uint64_t i, uint32_t, bool masked) { return masked ? keys[i] & T.g.key_mask : keys[i]; }
  __device__ static Lane stage_tile(const DevTable&, const uint8_t* __restrict__ base, int64_t tile_start, int64_t lo, int64_t hi, uint32_t* s_codes, uint32_t* s_inv) {
    return jfgpu::stage_tile(base, tile_start, lo, hi, s_codes, s_inv);
  }
  template <typename F>
  __device__ static void for_each_kmer(const DevTable& T, const Lane& L, F&& f) { jfgpu::for_each_kmer(T.g, L, [&](int j, uint64_t key) { f(j, key, true); }); }
  __device__ static Key text_key(const DevTable& T, const Lane& L, int j) {     // the k-mer as the text has it (no canonical form) ending at position j
    return (((((uint64_t)L.p2 << 32) | L.p1) << (2 * j + 2)) | (L.cur >> (30 - 2 * j))) & T.g.key_mask;
  }
  __device__ static uint32_t route_rank(bool valid, uint32_t owner, uint32_t* s_hist) { return valid ? atomicAdd(&s_hist[owner], 1u) : 0u; }
  __device__ static uint32_t admit_mask(const DevTable& T, const Lane& L) { return bloom_admit_mask(T.bloom, T.g, L); }
  __device__ static bool admits(const DevTable&, uint32_t mask, int j, Key) { return (mask >> j) & 1u; }
};

__device__ inline LaneWords stage_tile(const uint8_t* __restrict__ base, int64_t tile_start, int64_t lo, int64_t hi,
                                       uint32_t* s_codes, uint32_t* s_inv) {
  const int tid = threadIdx.x;
  uint32_t c, v;
  load_pack16(base, tile_start + 16 * tid, lo, hi, c, v);
  s_codes[tid + 2] = c; s_inv[tid + 2] = v;
  if(tid < 2) {
    uint32_t hc, hv;
    load_pack16(base, tile_start - 32 + 16 * tid, lo, hi, hc, hv);
    s_codes[tid] = hc; s_inv[tid] = hv;
  }
  lds_barrier();
  LaneWords L;
  L.cur = c;
  L.p1 = s_codes[tid + 1];
  L.p2 = s_codes[tid];
  L.inv48 = ((uint64_t)s_inv[tid] << 32) | ((uint64_t)s_inv[tid + 1] << 16) | v;
  return L;
}

// The same in two halves, so a kernel can issue the loads of its NEXT tile before it works on the
// current one: tile_fetch only loads (4 + 4 registers), tile_stage packs and publishes to LDS.
struct TileRaw { uint32_t w[4]; uint32_t h[4]; };
__device__ inline void raw16(const uint8_t* __restrict__ base, int64_t off, int64_t lo, int64_t hi, uint32_t w[4]) {
  w[0] = w[1] = w[2] = w[3] = 0;
  if(off + 16 <= lo || off >= hi || off < 0) return;
  if(off + 16 <= hi) load16(base + off, w);
  else for(int i = 0; i < 16 && off + i < hi; ++i) w[i >> 2] |= (uint32_t)base[off + i] << (8 * (i & 3));
}
__device__ inline void edges16(const uint32_t w[4], int64_t off, int64_t lo, int64_t hi, uint32_t& codes, uint32_t& inval) {
  if(off + 16 <= lo || off >= hi || off < 0) { codes = 0; inval = 0xFFFFu; return; }
  pack16(w, codes, inval);
  if(off < lo) inval |= (0xFFFFu << (16 - (int)(lo - off))) & 0xFFFFu;
  if(off + 16 > hi) inval |= (1u << (int)(off + 16 - hi)) - 1u;
}
__device__ inline TileRaw tile_fetch(const uint8_t* __restrict__ base, int64_t tile_start, int64_t lo, int64_t hi) {
  TileRaw R;
  raw16(base, tile_start + 16 * (int64_t)threadIdx.x, lo, hi, R.w);
  R.h[0] = R.h[1] = R.h[2] = R.h[3] = 0;
  if(threadIdx.x < 2) raw16(base, tile_start - 32 + 16 * (int64_t)threadIdx.x, lo, hi, R.h);
  return R;
}
__device__ inline LaneWords tile_stage(const TileRaw& R, int64_t tile_start, int64_t lo, int64_t hi, uint32_t* s_codes, uint32_t* s_inv) {
  const int tid = threadIdx.x;
  uint32_t c, v;
  edges16(R.w, tile_start + 16 * (int64_t)tid, lo, hi, c, v);
  s_codes[tid + 2] = c; s_inv[tid + 2] = v;
  if(tid < 2) {
    uint32_t hc, hv;
    edges16(R.h, tile_start - 32 + 16 * (int64_t)tid, lo, hi, hc, hv);
    s_codes[tid] = hc; s_inv[tid] = hv;
  }
  lds_barrier();
  LaneWords L;
  L.cur = c;
  L.p1 = s_codes[tid + 1];
  L.p2 = s_codes[tid];
  L.inv48 = ((uint64_t)s_inv[tid] << 32) | ((uint64_t)s_inv[tid + 1] << 16) | v;
  return L;
}

// ---- K2+K3 fused: count every k-mer of a contract buffer ----------------------
// base: 16-byte aligned; valid bytes are [lo, hi).
// op: 0 COUNT add(m, 1); 1 PRIME set(m) = claim with count 0; 2 UPDATE update_add(m, 1) (count_main.cc:152-184).
template <bool RETURNING, bool BLOOM>
__global__ __launch_bounds__(kBlock) void count_ascii_kernel(DevTable T, const uint8_t* __restrict__ base,
                                                             int64_t lo, int64_t hi, int op) {
  __shared__ uint64_t s_fwd[8 * 256];
  __shared__ uint32_t s_codes[kBlock + 2];
  __shared__ uint32_t s_inv[kBlock + 2];
  __shared__ int s_abort;
  load_tables_lds(s_fwd, T.fwd_tbl, T.g.nbytes);
  const int64_t n_tiles = (hi + kTilePos - 1) / kTilePos;
  uint32_t my_mers = 0;
  for(int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    // "Hash full" already raised by some block: the result is void, stop burning probes (the
    // host reports the error at jfgpu_sync).  One lane polls, the barrier makes it block-uniform
    // and also fences the previous iteration's LDS reads.
    if(threadIdx.x == 0)
      s_abort = __hip_atomic_load(&T.counters[CTR_FULL], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
    __syncthreads();
    if(s_abort) break;
    const LaneWords L = stage_tile(base, tile * kTilePos, lo, hi, s_codes, s_inv);
    // run-length merge of consecutive identical k-mers (homopolymers / short tandem
    // repeats are the heavy hitters of real data): one atomic per run, not per k-mer.
    uint64_t prev = 0; uint32_t run = 0;
    auto apply = [&](uint64_t key, uint32_t n) {
      if(op == 0) table_add<RETURNING>(T, s_fwd, key, n);
      else if(op == 1) table_add<RETURNING>(T, s_fwd, key, 0);
      else table_update_add<RETURNING>(T, s_fwd, key, n);
    };
    const uint32_t adm = BLOOM ? bloom_admit_mask(T.bloom, T.g, L) : 0xFFFFu;   // count --bc (count_main.cc:115-118); compiled out otherwise
    for_each_kmer(T.g, L, [&](int j, uint64_t key) {
      ++my_mers;
      if(BLOOM && !((adm >> j) & 1u)) return;
      if(run && key == prev) { ++run; return; }
      if(run) apply(prev, run);
      prev = key; run = 1;
    });
    if(run) apply(prev, run);
  }
  // one counter update per wave
  uint64_t w = my_mers;
  for(int o = 32; o > 0; o >>= 1) w += __shfl_down(w, o, 64);
  if((threadIdx.x & 63) == 0 && w) atomicAdd((unsigned long long*)&T.counters[CTR_MERS], (unsigned long long)w);
}

// ---- hash_counter::add on encoded keys, val == 1 and no is_new: the receive side of the multi-GPU exchange ----
// (the one-word fast path; every other add of keys is add_keys_kernel below)
template <bool RETURNING>
__global__ __launch_bounds__(kBlock) void add_keys_one_kernel(DevTable T, const uint64_t* __restrict__ keys, uint64_t n) {
  __shared__ uint64_t s_fwd[8 * 256];
  load_tables_lds(s_fwd, T.fwd_tbl, T.g.nbytes);
  __syncthreads();
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    table_add<RETURNING>(T, s_fwd, keys[i] & T.g.key_mask, 1);
}

// ---- cooperative size doubling (hash_counter::double_size, hash_counter.hpp:200-238) -------------
// Every entry of the old table is re-derived (slot -> key by the inverse tables) and inserted with its
// full count into the new, twice as large table (one more matrix row).  Hash tables are read through
// the caches here: growth is rare and the kernel is bound by the random inserts anyway.  Every key width (KeyOps).
template <class Table>
__global__ __launch_bounds__(kBlock) void rehash_kernel(Table old, Table neu, int have_ovf) {
  typedef KeyOps<Table> K;
  const TableGeom& g = K::geom(old);
  const uint64_t n = 1ull << g.lsize_l;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    typename K::Slot s;
    if(!K::load(old, i, s)) continue;
    const typename K::Key key = K::key(old, s, i & ~g.tile_mask);
    K::add_val(neu, neu.fwd_tbl, key, K::count(old, s, i, have_ovf));
  }
}

// ---- the kernels that are handed keys, kw words each (low first): every key width (KeyOps) ---------------------------
// hash_counter::add(key, val) on encoded mers (hash_counter.hpp:91-126)
template <class Table>
__global__ __launch_bounds__(kBlock) void add_keys_kernel(Table T, const uint64_t* __restrict__ keys, uint64_t n, uint32_t kw, uint64_t val,
                                                          uint8_t* __restrict__ is_new) {
  typedef KeyOps<Table> K;
  const uint64_t* H = K::stage_fwd(T);
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const bool nw = K::add_val(T, H, K::load_key(T, keys, i, kw, true), val);
    if(is_new) is_new[i] = nw ? 1 : 0;
  }
}

// hash_counter::update_add(key, 1): the receive side of the exchange in the UPDATE pass of count --if over shards
// (count_main.cc:152-184 with --gpus): only keys that are present are counted, a key of another shard is counted as misrouted.
template <class Table, bool RETURNING>
__global__ __launch_bounds__(kBlock) void update_keys_kernel(Table T, const uint64_t* __restrict__ keys, uint64_t n, uint32_t kw) {
  typedef KeyOps<Table> K;
  const uint64_t* H = K::stage_fwd(T);
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    K::template update_add<RETURNING>(T, H, K::load_key(T, keys, i, kw, true), 1);
}

// array_base::get_val_for_key (large_hash_array.hpp:354-372)
template <class Table>
__global__ __launch_bounds__(kBlock) void lookup_kernel(Table T, const uint64_t* __restrict__ keys, uint64_t n, uint32_t kw,
                                                        uint64_t* __restrict__ vals, uint8_t* __restrict__ found, int have_ovf) {
  typedef KeyOps<Table> K;
  const uint64_t* H = K::stage_fwd(T);
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t s = K::find(T, H, K::load_key(T, keys, i, kw, true));
    vals[i] = s == ~0ull ? 0 : K::count_at(T, s, have_ovf);
    if(found) found[i] = s != ~0ull;
  }
}

// ---- query: the count of every k-mer of a contract buffer, every key width (KeyOps) ----------------------------------
// query_from_sequence (sub_commands/query_main.cc:44-51; examples/query_per_sequence): mer_iterator over the sequence and
// array::get_val_for_key per k-mer, fused -- the tile loop of route_count_kernel with the look-up of lookup_kernel inside.
// The table is only read: no atomics, no counters.
// Output, indexed by the byte position p of the window's LAST base (p - lo of the aligned buffer): vals[p] the full count
// (0 where no k-mer ends or the key is absent) and, when flags is given, JFGPU_Q_MER | JFGPU_Q_FOUND | JFGPU_Q_REVCOMP.  Every
// entry of [0, hi - lo) is written, nothing else.  A lane's 16 positions are 128 bytes of vals and 16 of flags: eight and
// one 16-byte stores when the caller's buffers are aligned (lo == 0, vals and flags on 16 bytes), single entries otherwise
// and in the ragged last lane.
// One word: a lane's 16 look-ups do not wait for one another.  Sweep one hashes every window and issues the load of the
// first slot of its home bucket (KeyOps::find_begin, the registers of route_scatter_kernel's keys[j]); sweep two resolves
// them (find_end), probing on where the first slot was another key's.  The wider views roll once and look up as they go.
// A window whose key equals the previous position's takes its answer (homopolymers and short tandem repeats, the run
// merge of count_ascii_kernel).
// LDS: the forward tables and the tile's codes and invalid masks; static for one and two words, dynamic for NTable
// (query_lds_bytes).
constexpr uint32_t kQMer = 1, kQFound = 2, kQRevcomp = 4;      // JFGPU_Q_* (include/jfgpu.h)
struct QueryLds { uint64_t* fwd; uint32_t *codes, *inv; };
inline size_t query_lds_bytes(uint32_t nbytes, uint32_t halo_words) { return (size_t)nbytes * 256 * 8 + 2 * (kBlock + halo_words) * 4; }
template <class Table>
__device__ inline QueryLds query_lds(uint32_t nbytes) {
  typedef KeyOps<Table> K;
  constexpr uint32_t kStage = kBlock + K::kHaloWords;
  QueryLds S;
  if constexpr(K::kFwdLdsWords != 0) {
    __shared__ uint64_t s_fwd[K::kFwdLdsWords];
    __shared__ uint32_t s_codes[kStage];
    __shared__ uint32_t s_inv[kStage];
    S.fwd = s_fwd; S.codes = s_codes; S.inv = s_inv;
  } else {
    JF_DYN_LDS(s_raw);
    S.fwd = reinterpret_cast<uint64_t*>(s_raw);
    S.codes = reinterpret_cast<uint32_t*>(S.fwd + (size_t)nbytes * 256);
    S.inv = S.codes + kStage;
  }
  return S;
}

template <class Table>
__global__ __launch_bounds__(kBlock) void query_ascii_kernel(Table T, const uint8_t* __restrict__ base, int64_t lo, int64_t hi,
                                                             uint64_t* __restrict__ vals, uint8_t* __restrict__ flags, int have_ovf) {
  typedef KeyOps<Table> K;
  typedef typename K::Key Key;
  constexpr bool kTwoSweeps = sizeof(Key) == 8;
  const TableGeom& g = K::geom(T);
  const QueryLds S = query_lds<Table>(g.nbytes);
  load_tables_lds(S.fwd, T.fwd_tbl, g.nbytes);
  const bool aligned = lo == 0 && (((uintptr_t)vals | (uintptr_t)flags) & 15) == 0;
  const int64_t n_tiles = (hi + kTilePos - 1) / kTilePos;
  for(int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    __syncthreads();
    const typename K::Lane L = K::stage_tile(T, base, tile * kTilePos, lo, hi, S.codes, S.inv);     // contains a barrier
    // indexed by the unrolled position j (compile-time after unrolling) so these stay in VGPRs
    uint64_t v[kPerThread]; uint32_t fl[kPerThread / 4] = {0, 0, 0, 0};
    auto revcomp_bit = [&](int j, const Key& key) { return (g.canonical && !K::same_key(key, K::text_key(T, L, j))) ? kQRevcomp : 0u; };
    auto answer = [&](int j, uint64_t count, uint32_t bits) { v[j] = count; fl[j >> 2] |= bits << (8 * (j & 3)); };
    if constexpr(kTwoSweeps) {
      typename K::Probe pr[kPerThread]; Key prev = 0; uint32_t mer = 0, rc = 0, same = 0;
      K::for_each_kmer(T, L, [&](int j, const Key& key, bool) {
        mer |= 1u << j; rc |= (revcomp_bit(j, key) ? 1u : 0u) << j;
        if(j > 0 && ((mer >> (j - 1)) & 1u) && key == prev) { same |= 1u << j; return; }
        prev = key;
        pr[j] = K::find_begin(T, S.fwd, key);
      });
      uint64_t count = 0; uint32_t bits = 0;
#pragma unroll
      for(int j = 0; j < kPerThread; ++j) {
        if(!((mer >> j) & 1u)) { v[j] = 0; continue; }
        if(!((same >> j) & 1u)) {
          const uint64_t slot = K::find_end(T, pr[j]);
          bits = slot != ~0ull ? kQFound : 0u;
          count = slot != ~0ull ? full_count(T, pr[j].w, slot, have_ovf) : 0;
        }
        answer(j, count, kQMer | bits | (((rc >> j) & 1u) ? kQRevcomp : 0u));
      }
    } else {
#pragma unroll
      for(int j = 0; j < kPerThread; ++j) v[j] = 0;
      Key prev = Key(); int last = -2; uint64_t count = 0; uint32_t bits = 0;
      K::for_each_kmer(T, L, [&](int j, const Key& key, bool valid) {
        if(!valid) return;
        if(last != j - 1 || !K::same_key(key, prev)) {
          const uint64_t slot = K::find(T, S.fwd, key);
          bits = slot != ~0ull ? kQFound : 0u;
          count = slot != ~0ull ? K::count_at(T, slot, have_ovf) : 0;
          prev = key;
        }
        last = j;
        answer(j, count, kQMer | bits | revcomp_bit(j, key));
      });
    }
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

// ---- multi-GPU routing: a contract buffer's k-mers grouped by owner, every key width (KeyOps) -------------------------
// The sender's two passes (route_buffer in jfgpu.hip: the key path of abi_comm.inl, jfgpu_partition_ascii_dev).  The owner of a
// k-mer is pos >> lsize_l under the shard's global matrix.  Pass A counts the k-mers per owner; the host turns the counts into
// cursors (the regions' offsets); pass B writes every k-mer into its owner's region as kw little-endian words, the layout of
// jfgpu_add_keys.  Counts and cursors are in k-mers.  A workgroup counts in LDS and sends one global atomic per owner: per
// buffer in pass A, per tile in pass B, where it reserves the tile's share of each region.
// BLOOM: count --bc with --gpus -- the sender asks its copy of the Bloom counter, what it does not admit never travels.  The
// counter is read-only here, so both passes get the same answers.
// LDS: the forward tables, s_base (pass B), s_hist, and the tile's codes and invalid masks.  Static where the view stages its
// tables statically; NTable's 64 KiB of tables make it dynamic, route_lds_bytes() for both of its kernels.
struct RouteLds { uint64_t* fwd; unsigned long long* base; uint32_t *hist, *codes, *inv; };
constexpr uint32_t kRouteOwners = 256;                     // s_hist / s_base: shard_bits <= 8
inline size_t route_lds_bytes(uint32_t nbytes, uint32_t halo_words) { return (size_t)nbytes * 256 * 8 + kRouteOwners * (8 + 4) + 2 * (kBlock + halo_words) * 4; }
template <class Table, bool SCATTER>
__device__ inline RouteLds route_lds(uint32_t nbytes) {
  typedef KeyOps<Table> K;
  constexpr uint32_t kStage = kBlock + K::kHaloWords;
  static_assert(16 * K::kHaloWords >= 4 * sizeof(typename K::Key) - 1, "the halo holds the k - 1 bases before a tile, for the view's longest k");
  RouteLds S;
  if constexpr(K::kFwdLdsWords != 0) {
    __shared__ uint64_t s_fwd[K::kFwdLdsWords];
    __shared__ uint32_t s_codes[kStage];
    __shared__ uint32_t s_inv[kStage];
    __shared__ uint32_t s_hist[kRouteOwners];
    S.fwd = s_fwd; S.codes = s_codes; S.inv = s_inv; S.hist = s_hist; S.base = nullptr;
    if constexpr(SCATTER) { __shared__ unsigned long long s_base[kRouteOwners]; S.base = s_base; }
  } else {
    JF_DYN_LDS(s_raw);
    S.fwd = reinterpret_cast<uint64_t*>(s_raw);
    S.base = reinterpret_cast<unsigned long long*>(S.fwd + (size_t)nbytes * 256);
    S.hist = reinterpret_cast<uint32_t*>(S.base + kRouteOwners);
    S.codes = S.hist + kRouteOwners;
    S.inv = S.codes + kStage;
  }
  return S;
}

// Pass A: how many k-mers of this buffer belong to each shard.
// (A BLOOM kernel leaves f at a k-mer its counter does not admit: the views that take a filter call f for the valid windows
// only and rank without a ballot, so no lane is missed by one.)
template <class Table, bool BLOOM>
__global__ __launch_bounds__(kBlock) void route_count_kernel(Table T, const uint8_t* __restrict__ base, int64_t lo, int64_t hi,
                                                             unsigned long long* __restrict__ shard_counts) {
  typedef KeyOps<Table> K;
  const TableGeom& g = K::geom(T);
  const RouteLds S = route_lds<Table, false>(g.nbytes);
  load_tables_lds(S.fwd, T.fwd_tbl, g.nbytes);
  const uint32_t n_shards = 1u << g.shard_bits;
  for(uint32_t i = threadIdx.x; i < n_shards; i += blockDim.x) S.hist[i] = 0;
  const int64_t n_tiles = (hi + kTilePos - 1) / kTilePos;
  for(int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    __syncthreads();
    const typename K::Lane L = K::stage_tile(T, base, tile * kTilePos, lo, hi, S.codes, S.inv);
    uint32_t adm = 0;
    if constexpr(BLOOM) adm = K::admit_mask(T, L);
    K::for_each_kmer(T, L, [&](int j, const typename K::Key& key, bool valid) {
      if constexpr(BLOOM) if(!K::admits(T, adm, j, key)) return;
      K::route_rank(valid, valid ? K::owner(T, S.fwd, key) : 0u, S.hist);
    });
  }
  __syncthreads();
  for(uint32_t i = threadIdx.x; i < n_shards; i += blockDim.x)
    if(S.hist[i]) atomicAdd(&shard_counts[i], (unsigned long long)S.hist[i]);
}

// Pass B: write each k-mer into its shard's region.  cursors[s] starts at the region's offset; a block reserves its share
// with one atomic per (tile, shard).  Two sweeps over the lane's windows, ranks and then stores.  Keys of one word are kept in
// registers between the sweeps; wider ones are rolled again (the re-rolled form costs the one-word kernel a wave per SIMD,
// the kept form the wider ones their registers: profiles/route_kernel_resources.txt).
template <class Table, bool BLOOM>
__global__ __launch_bounds__(kBlock) void route_scatter_kernel(Table T, const uint8_t* __restrict__ base, int64_t lo, int64_t hi,
                                                               unsigned long long* __restrict__ cursors, uint64_t* __restrict__ out, uint32_t kw) {
  typedef KeyOps<Table> K;
  typedef typename K::Key Key;
  constexpr bool kKeepKeys = sizeof(Key) == 8;
  const TableGeom& g = K::geom(T);
  const RouteLds S = route_lds<Table, true>(g.nbytes);
  load_tables_lds(S.fwd, T.fwd_tbl, g.nbytes);
  const uint32_t n_shards = 1u << g.shard_bits;
  const uint32_t stride = K::kKeyWords ? K::kKeyWords : kw;
  const int64_t n_tiles = (hi + kTilePos - 1) / kTilePos;
  for(int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    __syncthreads();
    for(uint32_t i = threadIdx.x; i < n_shards; i += blockDim.x) S.hist[i] = 0;
    const typename K::Lane L = K::stage_tile(T, base, tile * kTilePos, lo, hi, S.codes, S.inv);     // contains a barrier
    // indexed by the unrolled position j (compile-time after unrolling) so these stay in VGPRs
    Key keys[kKeepKeys ? kPerThread : 1]; uint32_t sh[kPerThread], rank[kPerThread], routed = 0;
    uint32_t adm = 0;
    if constexpr(BLOOM) adm = K::admit_mask(T, L);
    K::for_each_kmer(T, L, [&](int j, const Key& key, bool valid) {
      if constexpr(BLOOM) if(!K::admits(T, adm, j, key)) return;
      if constexpr(kKeepKeys) keys[j] = key;
      sh[j] = valid ? K::owner(T, S.fwd, key) : 0u;
      rank[j] = K::route_rank(valid, sh[j], S.hist);
      routed |= (uint32_t)valid << j;
    });
    __syncthreads();
    for(uint32_t i = threadIdx.x; i < n_shards; i += blockDim.x)
      S.base[i] = S.hist[i] ? atomicAdd(&cursors[i], (unsigned long long)S.hist[i]) : 0ull;
    __syncthreads();
    auto store = [&](int j, const Key& key, bool routes) { if(routes) K::store_key(out + (uint64_t)stride * (S.base[sh[j]] + rank[j]), key, kw); };
    if constexpr(kKeepKeys) {
#pragma unroll
      for(int j = 0; j < kPerThread; ++j) store(j, keys[j], (routed >> j) & 1u);
    } else K::for_each_kmer(T, L, [&](int j, const Key& key, bool valid) { store(j, key, BLOOM ? (routed >> j) & 1u : valid); });
  }
}

// ---- stats (stats_main.cc:33-46) ---------------------------------------------------
// out: [0] unique [1] distinct [2] total [3] max
__global__ __launch_bounds__(kBlock) void stats_kernel(DevTable T, uint64_t lower, uint64_t upper, int have_ovf,
                                                       unsigned long long* __restrict__ out) {
  const uint64_t n = 1ull << T.g.lsize_l;
  uint64_t uniq = 0, dist = 0, tot = 0, mx = 0;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t w = slot_ld(T, i);
    if(!w) continue;
    const uint64_t c = full_count(T, w, i, have_ovf);
    if(c < lower || c > upper) continue;
    uniq += (c == 1); ++dist; tot += c; mx = c > mx ? c : mx;
  }
  for(int o = 32; o > 0; o >>= 1) {
    uniq += __shfl_down(uniq, o, 64); dist += __shfl_down(dist, o, 64); tot += __shfl_down(tot, o, 64);
    const uint64_t m2 = __shfl_down(mx, o, 64); mx = m2 > mx ? m2 : mx;
  }
  if((threadIdx.x & 63) == 0) {
    if(uniq) atomicAdd(&out[0], (unsigned long long)uniq);
    if(dist) atomicAdd(&out[1], (unsigned long long)dist);
    if(tot) atomicAdd(&out[2], (unsigned long long)tot);
    if(mx) atomicMax(&out[3], (unsigned long long)mx);
  }
}

// ---- content digest (at-scale parity) -----------------------------------------
// An order-independent checksum of the {k-mer -> count} multiset: per entry h = mix(..mix(mix(seed ^ w0) ^ w1).. ^ count)
// over the key's little-endian 64-bit words, then out[0] += 1, out[1] += count, out[2] += h, out[3] ^= h (all mod 2^64).
// The reference driver (oracle/ref_drivers/ref_jf.cc, `count --digest` / `digest`) computes the same four numbers from the
// reference's own table, so two runs over 10 Gbp are compared without writing or sorting 86 GB of records.
__device__ __host__ inline uint64_t digest_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
constexpr uint64_t kDigestSeed = 0x9E3779B97F4A7C15ull;

__device__ inline void digest_reduce(uint64_t n, uint64_t tot, uint64_t sum, uint64_t x, unsigned long long* __restrict__ out) {
  for(int o = 32; o > 0; o >>= 1) {
    n += __shfl_down(n, o, 64); tot += __shfl_down(tot, o, 64); sum += __shfl_down(sum, o, 64); x ^= __shfl_down(x, o, 64);
  }
  if((threadIdx.x & 63) == 0 && n) {
    atomicAdd(&out[0], (unsigned long long)n); atomicAdd(&out[1], (unsigned long long)tot);
    atomicAdd(&out[2], (unsigned long long)sum); atomicXor(&out[3], (unsigned long long)x);
  }
}

__global__ __launch_bounds__(kBlock) void digest_kernel(DevTable T, uint64_t lower, uint64_t upper, int have_ovf,
                                                        unsigned long long* __restrict__ out) {
  __shared__ uint64_t s_inv[8 * 256];
  load_tables_lds(s_inv, T.inv_tbl, T.g.nbytes);
  __syncthreads();
  const uint64_t n = 1ull << T.g.lsize_l;
  uint64_t cnt = 0, tot = 0, sum = 0, x = 0;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t w = slot_ld(T, i);
    if(!w) continue;
    const uint64_t c = full_count(T, w, i, have_ovf);
    if(c < lower || c > upper) continue;
    const uint64_t key = slot_key(T.g, s_inv, w, i & ~T.g.tile_mask);
    const uint64_t h = digest_mix(digest_mix(kDigestSeed ^ key) ^ c);
    ++cnt; tot += c; sum += h; x ^= h;
  }
  digest_reduce(cnt, tot, sum, x, out);
}

// ---- histo (histo_main.cc:34-45) -----------------------------------------------------
constexpr uint32_t kHistoLds = 8192;  // buckets privatised per block
__global__ __launch_bounds__(kBlock) void histo_kernel(DevTable T, uint64_t hbase, uint64_t hceil, uint64_t inc,
                                                       uint64_t nb, int have_ovf, unsigned long long* __restrict__ histo) {
  __shared__ uint32_t s_h[kHistoLds];
  const uint32_t nl = nb < kHistoLds ? (uint32_t)nb : kHistoLds;
  for(uint32_t i = threadIdx.x; i < nl; i += blockDim.x) s_h[i] = 0;
  __syncthreads();
  const uint64_t n = 1ull << T.g.lsize_l;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t w = slot_ld(T, i);
    if(!w) continue;
    const uint64_t c = full_count(T, w, i, have_ovf);
    uint64_t b;
    if(c < hbase) b = 0; else if(c > hceil) b = nb - 1; else b = (c - hbase) / inc;
    if(b < nl) atomicAdd(&s_h[(uint32_t)b], 1u); else atomicAdd(&histo[b], 1ull);
  }
  __syncthreads();
  for(uint32_t i = threadIdx.x; i < nl; i += blockDim.x)
    if(s_h[i]) atomicAdd(&histo[i], (unsigned long long)s_h[i]);
}

// ---- sorted dump ------------------------------------------------------------------------
// Pass 1: records per tile after the [lower, upper] filter.
__global__ __launch_bounds__(kBlock) void tile_count_kernel(DevTable T, uint64_t lower, uint64_t upper, int have_ovf,
                                                            uint64_t n_tiles, uint32_t* __restrict__ tile_counts) {
  __shared__ uint32_t s_sum[kBlock / 64];
  const uint32_t tsz = 1u << T.g.tile_bits;
  for(uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t tb = tile << T.g.tile_bits;
    uint32_t c = 0;
    for(uint32_t i = threadIdx.x; i < tsz; i += blockDim.x) {
      const uint64_t w = slot_ld(T, tb + i);
      if(!w) continue;
      const uint64_t cnt = full_count(T, w, tb + i, have_ovf);
      c += (cnt >= lower && cnt <= upper);
    }
    for(int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = c;
    __syncthreads();
    if(threadIdx.x == 0) { uint32_t s = 0; for(int i = 0; i < kBlock / 64; ++i) s += s_sum[i]; tile_counts[tile] = s; }
    __syncthreads();
  }
}

// Pass 2: one block per tile.  Load the tile into LDS, bitonic-sort by tag (== (pos, key)
// order, mer_heap.hpp:26-30), rebuild each key with the inverse tables and emit
// fixed-width records (binary_dumper.hpp:36-40) at the tile's record offset.
// Dynamic LDS: tsz * 8 (words) + tsz * 2 (slot index) + nbytes * 2048 (inverse tables).
__global__ __launch_bounds__(kBlock) void dump_tiles_kernel(DevTable T, uint64_t lower, uint64_t upper, int have_ovf,
                                                            uint64_t tile0, uint64_t n_tiles,
                                                            const uint64_t* __restrict__ tile_offsets,  // record offset of tile (relative to tile0's)
                                                            uint8_t* __restrict__ out, uint32_t key_bytes, uint32_t val_bytes) {
  JF_DYN_LDS(s_raw);
  const uint32_t tsz = 1u << T.g.tile_bits;
  uint64_t* s_w = reinterpret_cast<uint64_t*>(s_raw);
  uint64_t* s_invt = s_w + tsz;
  uint16_t* s_idx = reinterpret_cast<uint16_t*>(s_invt + T.g.nbytes * 256);
  load_tables_lds(s_invt, T.inv_tbl, T.g.nbytes);
  const uint64_t tagmask = T.g.occ_bit - 1;
  const uint64_t SENT = ~T.g.occ_bit;      // no stored slot equals it (they all have the occupied bit), and it sorts after every tag
  const uint64_t maxval = val_bytes >= 8 ? ~0ull : ((1ull << (8 * val_bytes)) - 1);
  const uint32_t rec = key_bytes + val_bytes;
  for(uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint64_t tile = tile0 + t;
    const uint64_t tb = tile << T.g.tile_bits;
    __syncthreads();
    for(uint32_t i = threadIdx.x; i < tsz; i += blockDim.x) {
      uint64_t w = slot_ld(T, tb + i);
      uint64_t sk = SENT;
      if(w) {
        const uint64_t cnt = full_count(T, w, tb + i, have_ovf);
        if(cnt >= lower && cnt <= upper) sk = w;
      }
      s_w[i] = sk; s_idx[i] = (uint16_t)i;
    }
    __syncthreads();
    // bitonic sort ascending on (word & tagmask), sentinels last
    for(uint32_t size = 2; size <= tsz; size <<= 1) {
      for(uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
        for(uint32_t i = threadIdx.x; i < tsz / 2; i += blockDim.x) {
          const uint32_t lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1));
          const uint32_t hi = lo | stride;
          const bool up = (lo & size) == 0;
          const uint64_t a = s_w[lo], b = s_w[hi];
          const uint64_t ka = a == SENT ? SENT : (a & tagmask), kb = b == SENT ? SENT : (b & tagmask);
          if((ka > kb) == up) {
            s_w[lo] = b; s_w[hi] = a;
            const uint16_t ia = s_idx[lo]; s_idx[lo] = s_idx[hi]; s_idx[hi] = ia;
          }
        }
        __syncthreads();
      }
    }
    uint8_t* dst0 = out + tile_offsets[t] * rec;
    for(uint32_t i = threadIdx.x; i < tsz; i += blockDim.x) {
      const uint64_t w = s_w[i];
      if(w == SENT) continue;
      const uint64_t key = slot_key(T.g, s_invt, w, tb);
      uint64_t cnt = slot_count(T.g, w);
      if(have_ovf) cnt += ovf_get(T, tb + s_idx[i]) << T.g.cnt_bits;
      if(cnt > maxval) cnt = maxval;
      uint8_t* d = dst0 + (uint64_t)i * rec;
      for(uint32_t b = 0; b < key_bytes; ++b) d[b] = (uint8_t)(key >> (8 * b));
      for(uint32_t b = 0; b < val_bytes; ++b) d[key_bytes + b] = (uint8_t)(cnt >> (8 * b));
    }
  }
}

// ---- the same passes over multi-word keys (WideTable, NTable) ------------------------------------------------
// stats / histo / tile counts / content digest as one strided scan (the one-word kernels above are shaped for k <= 32:
// tables in LDS, a privatised histogram, one block per tile).  The counting scans take KeyOps::occupied, the digest needs
// the key and takes the whole slot.
enum { SCAN_STATS = 0, SCAN_HISTO = 1, SCAN_TILES = 2, SCAN_DIGEST = 3 };   // out[0..3] = unique, distinct, total, max | histogram | tile_counts | digest
template <class Table>
__global__ __launch_bounds__(kBlock) void scan_kernel(Table T, int what, uint64_t lower, uint64_t upper, int have_ovf,
                                                      uint64_t hbase, uint64_t hceil, uint64_t hinc, uint64_t nb,
                                                      unsigned long long* __restrict__ out, uint32_t* __restrict__ tile_counts) {
  typedef KeyOps<Table> K;
  const TableGeom& g = K::geom(T);
  const uint64_t n = 1ull << g.lsize_l;
  uint64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    typename K::Slot s;
    if(!(what == SCAN_DIGEST ? K::load(T, i, s) : K::occupied(T, i, s))) continue;
    const uint64_t c = K::count(T, s, i, have_ovf);
    if(what == SCAN_HISTO) {
      uint64_t b;
      if(c < hbase) b = 0; else if(c > hceil) b = nb - 1; else b = (c - hbase) / hinc;
      atomicAdd(&out[b], 1ull);
      continue;
    }
    if(c < lower || c > upper) continue;
    if(what == SCAN_TILES) { atomicAdd(&tile_counts[i >> g.tile_bits], 1u); continue; }
    if(what == SCAN_DIGEST) {
      const uint64_t h = K::digest(T, K::key(T, s, i & ~g.tile_mask), c);
      ++a0; a1 += c; a2 += h; a3 ^= h;
      continue;
    }
    a0 += (c == 1); ++a1; a2 += c; a3 = c > a3 ? c : a3;
  }
  if(what == SCAN_DIGEST) { digest_reduce(a0, a1, a2, a3, out); return; }
  if(what == SCAN_STATS) {
    for(int o = 32; o > 0; o >>= 1) {
      a0 += __shfl_down(a0, o, 64); a1 += __shfl_down(a1, o, 64); a2 += __shfl_down(a2, o, 64);
      const uint64_t m2 = __shfl_down(a3, o, 64); a3 = m2 > a3 ? m2 : a3;
    }
    if((threadIdx.x & 63) == 0) {
      if(a0) atomicAdd(&out[0], (unsigned long long)a0);
      if(a1) atomicAdd(&out[1], (unsigned long long)a1);
      if(a2) atomicAdd(&out[2], (unsigned long long)a2);
      if(a3) atomicMax(&out[3], (unsigned long long)a3);
    }
  }
}

// Sorted dump of slots of NW = KeyOps::kSlotWords words { lo words ..., hi }: one block per tile, bitonic sort in LDS on
// the tag (masked hi word, then the lo words from the most significant) == (pos, key) order (mer_heap.hpp:26-30), keys
// rebuilt through the inverse tables (read through the caches), records as binary_dumper.hpp:36-40 lays them out.
// Dynamic LDS: tsz * 8 * NW (word q of entry i at s_w[q * tsz + i]) + tsz * 2 (slot index): 8192 x 16 B = 128 KiB + 16 KiB
// for two-word keys, 2048 x 32 B = 64 KiB + 4 KiB for three and four.
template <class Table>
__global__ __launch_bounds__(kBlock) void dump_tiles_words_kernel(Table T, uint64_t lower, uint64_t upper, int have_ovf,
                                                                  uint64_t tile0, uint64_t n_tiles, const uint64_t* __restrict__ tile_offsets,
                                                                  uint8_t* __restrict__ out, uint32_t key_bytes, uint32_t val_bytes) {
  typedef KeyOps<Table> K;
  constexpr int NW = K::kSlotWords;
  JF_DYN_LDS(s_raw);
  const TableGeom& g = K::geom(T);
  const uint32_t tsz = 1u << g.tile_bits;
  uint64_t* s_w = reinterpret_cast<uint64_t*>(s_raw);
  uint64_t* s_hi = s_w + (NW - 1) * (size_t)tsz;
  uint16_t* s_idx = reinterpret_cast<uint16_t*>(s_w + NW * (size_t)tsz);
  const uint64_t tagmask = g.occ_bit - 1, SENT = ~g.occ_bit;     // (a stored hi word has the occupied bit: a saturated count field over an all-ones tag is not the sentinel)
  const uint64_t maxval = val_bytes >= 8 ? ~0ull : ((1ull << (8 * val_bytes)) - 1);
  const uint32_t rec = key_bytes + val_bytes;
  for(uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint64_t tb = (tile0 + t) << g.tile_bits;
    __syncthreads();
    for(uint32_t i = threadIdx.x; i < tsz; i += blockDim.x) {
      const uint64_t* sp = &T.slots[NW * (tb + i)];
      typename K::Slot s;
      uint64_t kh = SENT;
      if(K::occupied(T, tb + i, s)) {
        const uint64_t c = K::count(T, s, tb + i, have_ovf);
        if(c >= lower && c <= upper) kh = sp[NW - 1];
      }
#pragma unroll
      for(int q = 0; q < NW - 1; ++q) s_w[q * tsz + i] = sp[q];
      s_hi[i] = kh; s_idx[i] = (uint16_t)i;
    }
    __syncthreads();
    for(uint32_t size = 2; size <= tsz; size <<= 1) {
      for(uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
        for(uint32_t i = threadIdx.x; i < tsz / 2; i += blockDim.x) {
          const uint32_t l = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), h = l | stride;
          const bool up = (l & size) == 0;
          const uint64_t ah = s_hi[l], bh = s_hi[h];
          const uint64_t ka = ah == SENT ? SENT : (ah & tagmask), kb = bh == SENT ? SENT : (bh & tagmask);
          bool gt = ka > kb;
          if(ka == kb) {
#pragma unroll
            for(int q = NW - 2; q >= 0; --q) { const uint64_t x = s_w[q * tsz + l], y = s_w[q * tsz + h]; if(x != y) { gt = x > y; break; } }
          }
          if(gt == up) {
#pragma unroll
            for(int q = 0; q < NW; ++q) { const uint64_t x = s_w[q * tsz + l]; s_w[q * tsz + l] = s_w[q * tsz + h]; s_w[q * tsz + h] = x; }
            const uint16_t ia = s_idx[l]; s_idx[l] = s_idx[h]; s_idx[h] = ia;
          }
        }
        __syncthreads();
      }
    }
    uint8_t* dst0 = out + tile_offsets[t] * rec;
    for(uint32_t i = threadIdx.x; i < tsz; i += blockDim.x) {
      if(s_hi[i] == SENT) continue;
      uint64_t sl[NW];
#pragma unroll
      for(int q = 0; q < NW; ++q) sl[q] = s_w[q * tsz + i];
      const typename K::Slot s = K::slot_of(sl);
      const typename K::Key key = K::key(T, s, tb);
      uint64_t cnt = K::count(T, s, tb + s_idx[i], have_ovf);
      if(cnt > maxval) cnt = maxval;
      uint8_t* dd = dst0 + (uint64_t)i * rec;
      for(uint32_t b = 0; b < key_bytes; ++b) dd[b] = K::key_byte(key, b);
      for(uint32_t b = 0; b < val_bytes; ++b) dd[key_bytes + b] = (uint8_t)(cnt >> (8 * b));
    }
  }
}

// ---- synthetic reads (generate_sequence-like: iid uniform bases) ---------------------------
__device__ inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__global__ __launch_bounds__(kBlock) void gen_reads_kernel(uint8_t* __restrict__ out, uint64_t first_read, uint64_t n_reads,
                                                           uint32_t read_len, uint64_t seed) {
  const uint64_t stride = (uint64_t)read_len + 1;
  const uint64_t total = n_reads * stride;
  for(uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v * 16 < total; v += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p0 = v * 16;
    uint64_t r = p0 / stride; uint32_t off = (uint32_t)(p0 - r * stride);
    uint32_t w[4] = {0, 0, 0, 0};
    uint64_t draw = 0; uint64_t draw_id = ~0ull;
    for(int i = 0; i < 16; ++i) {
      uint32_t ch = 0;
      if(p0 + i < total) {
        if(off == read_len) ch = 'N';
        else {
          const uint64_t id = (first_read + r) * 64 + (off >> 5);   // 32 bases per draw
          if(id != draw_id) { draw_id = id; draw = mix64(mix64(seed + 0x9E3779B97F4A7C15ull * (id + 1))); }
          ch = (uint32_t)("ACGT"[(draw >> (2 * (off & 31))) & 3]);
        }
      }
      w[i >> 2] |= ch << (8 * (i & 3));
      if(++off == stride) { off = 0; ++r; }
    }
    if(p0 + 16 <= total) *reinterpret_cast<uint4*>(out + p0) = make_uint4(w[0], w[1], w[2], w[3]);
    else for(int i = 0; i < 16 && p0 + i < total; ++i) out[p0 + i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  }
}

// Distribution "G" of BASELINE.md section 3: reads sampled at uniform positions and strands from a uniform random
// genome (never materialised: base g of the genome is a pure function of (seed, g)), with iid substitutions.
// Same output layout as gen_reads_kernel (read_len bases + one 'N' per read), counter-based, any slice reproducible.
__device__ inline uint32_t genome_base(uint64_t gseed, uint64_t g) {
  const uint64_t d = mix64(mix64(gseed + 0x9E3779B97F4A7C15ull * ((g >> 5) + 1)));
  return (uint32_t)(d >> (2 * (g & 31))) & 3u;
}
__global__ __launch_bounds__(kBlock) void gen_genome_reads_kernel(uint8_t* __restrict__ out, uint64_t first_read, uint64_t n_reads,
                                                                  uint32_t read_len, uint64_t genome_len, uint32_t sub_per_64k,
                                                                  uint64_t seed) {
  const uint64_t stride = (uint64_t)read_len + 1;
  const uint64_t total = n_reads * stride;
  const uint64_t gseed = mix64(seed ^ 0x67656E6F6D65ull);
  for(uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v * 16 < total; v += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p0 = v * 16;
    uint64_t r = p0 / stride; uint32_t off = (uint32_t)(p0 - r * stride);
    uint32_t w[4] = {0, 0, 0, 0};
    uint64_t rid = ~0ull, pos = 0; bool rev = false;
    for(int i = 0; i < 16; ++i) {
      uint32_t ch = 0;
      if(p0 + i < total) {
        if(off == read_len) ch = 'N';
        else {
          if(r != rid) {
            rid = r;
            const uint64_t h = mix64(mix64(seed + 0xD1B54A32D192ED03ull * (first_read + r + 1)));
            pos = (h >> 1) % (genome_len - read_len + 1); rev = (h & 1) != 0;
          }
          uint32_t b = rev ? 3u - genome_base(gseed, pos + (read_len - 1 - off)) : genome_base(gseed, pos + off);
          const uint64_t e = mix64(seed + 0xA24BAED4963EE407ull * ((first_read + r) * 4096 + off + 1));   // substitution draw of this base
          if((uint32_t)(e & 0xFFFFu) < sub_per_64k) b = (b + 1 + (uint32_t)((e >> 16) % 3)) & 3u;
          ch = (uint32_t)("ACGT"[b]);
        }
      }
      w[i >> 2] |= ch << (8 * (i & 3));
      if(++off == stride) { off = 0; ++r; }
    }
    if(p0 + 16 <= total) *reinterpret_cast<uint4*>(out + p0) = make_uint4(w[0], w[1], w[2], w[3]);
    else for(int i = 0; i < 16 && p0 + i < total; ++i) out[p0 + i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  }
}

// ---- random-access roofline probes (R_gups) ------------------------------------
// mode 0: fire-and-forget atomicAdd   mode 1: returning atomicAdd   mode 2: atomicCAS(0 -> x)
// mode 3: plain load + dependent fire-and-forget atomicAdd
__global__ __launch_bounds__(kBlock) void gups_kernel(uint64_t* __restrict__ tab, uint64_t mask, uint64_t n, int mode,
                                                      uint64_t seed, unsigned long long* __restrict__ sink) {
  uint64_t acc = 0;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t s = mix64(seed + i * 0x9E3779B97F4A7C15ull) & mask;
    unsigned long long* a = (unsigned long long*)&tab[s];
    if(mode == 0) __hip_atomic_fetch_add(a, 1ull << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if(mode == 1) acc += atomicAdd(a, 1ull << 32);
    else if(mode == 2) acc += atomicCAS(a, 0ull, (unsigned long long)(i | 1));
    else { const uint64_t v = tab[s]; __hip_atomic_fetch_add(a, (1ull << 32) + (v & 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  }
  if(acc == 0x123456789ull) atomicAdd(sink, 1ull);
}

}  // namespace jfgpu
