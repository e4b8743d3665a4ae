// jellyfish_amd/csrc/jfgpu.hip -- C ABI (include/jfgpu.h) over the gfx950 kernels.
//
// Host-side role in the reference: the part of sub_commands/count_main.cc that
// owns the table (mer_hash ctor, :275), drives the counting threads (:331-333)
// and hands the table to the dumper (:349-355).  Here the "threads" are HIP
// kernels enqueued on one stream per table; there is no CPU fallback.
// Who owns what on the host: hip_own.hpp (owners in handles, raw pointers only inside the structs handed to kernels).
// Kernels with dynamic LDS are launched through launch_lds (hip_launch.hpp), which raises the kernel's limit on this device.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <array>
#include <chrono>
#include <memory>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/jfgpu.h"
#include "gf2_matrix.hpp"
#include "tuning.hpp"
#include "kernels.hip.hpp"
#include "kernels_part.hip.hpp"
#include "kernels_tile.hip.hpp"
#include "kernels_p1ring.hip.hpp"
#include "kernels_bloom.hip.hpp"
#include "kernels_bloom_part.hip.hpp"
#include "kernels_wide.hip.hpp"
#include "kernels_wide_part.hip.hpp"
#include "kernels_nword.hip.hpp"
#include "kernels_nword_part.hip.hpp"
#include "kernels_bloom_query.hip.hpp"
#include "kernels_parse.hip.hpp"
#include "kernels_bgzf.hip.hpp"
#include "kernels_stream.hip.hpp"
#include "kernels_merge.hip.hpp"
#include "kernels_sorted.hip.hpp"
#include "kernels_text.hip.hpp"
#include "kernels_qtext.hip.hpp"
#include "kernels_comm.hip.hpp"

using namespace jfgpu;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if(e_ != hipSuccess)                                                                      \
      return fail(e_ == hipErrorOutOfMemory ? JFGPU_E_ALLOC : (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice ? JFGPU_E_NO_DEVICE : JFGPU_E_HIP), \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                          \
  } while(0)

constexpr uint64_t kDefaultSeed = 0x6A656C6C79666973ull;  // "jellyfis"
constexpr size_t kStageBytes = 64u << 20;                  // host->device staging chunk
constexpr int kNumProf = 9;   // 0 count 1 add_keys 2 shard-partition 3 lookup 4 P1 5 P2 6 tile-insert 7 items-direct 8 query
enum Mode { MODE_AUTO = 0, MODE_DIRECT = 1, MODE_PARTITIONED = 2 };

// Entries of the count-overflow side table of a small table (1 MiB): counts beyond the in-slot field are rare in k-mer
// counting, but hash_counter::add(key, huge value) -- what the reference's unit tests do -- needs one per key.
constexpr uint64_t kMinOvf = 1ull << 16;

struct PendingBatch {
  void* items; uint64_t* off; uint64_t cap_items;
  uint32_t gran_cap = 0;                      // > 0: single-pass ("granule") batch, items per bucket region; off is in pair format
  unsigned long long* tot = nullptr;          // granule batch: exact items per bucket
  uint64_t input_bytes = 0;                   // sequence bytes this batch was made from (0: encoded keys)
  uint64_t bound = 0;                         // what ensure_capacity charged for this batch (an upper bound on its k-mers; 0: not charged)
};

struct ProfSpan { hipEvent_t a, b; int which; uint64_t units; };   // (events of the table's pool: get_event)

}  // namespace

#include "hip_own.hpp"
#include "hip_launch.hpp"

struct jfgpu_table {
  jfgpu_params params{};
  TableGeom g{};
  Gf2Matrix matrix;
  int device = 0;
  int n_cu = 256;
  Stream stream, stream2;        // (before every buffer used on them: the buffers go first.  stream2: part_flush_t's second one, on demand)
  // what kernels receive (DevTable, WideTable, NTable) holds raw pointers, set from the owners here
  DevTable dt{};
  DevBuf<uint8_t> slots, dirty;
  DevBuf<uint64_t> ovf_key, ovf_cnt, counters;
  DevBuf<DevTable> d_dt;         // a copy of dt in device memory for kernels that call out of line with it (refreshed before every such launch)
  DevBuf<uint64_t> d_fwd, d_inv;
  int failed = 0; std::string failed_msg;   // a flush failed: every call reports it until jfgpu_clear (host_partition.inl: part_flush)
  uint64_t ovf_cap = 0;
  // what the side table may have to hold: an entry needs 2^cnt_bits occurrences of its key, or one add of a large value
  uint64_t occ_bound = 0, bigval_bound = 0;      // upper bounds since the last clear (ensure_ovf)
  uint64_t flushes_plain = 0, flushes_heavy = 0; // tile-kernel instantiation chosen per flush launch (jfgpu_get_counters)
  // which partition kernels ran since the last clear (jfgpu_get_counters 10..15): P2 launches by kind -- loader / storer
  // rings, shared rings, the sort-based single pass, the exact count + scatter -- and P1 launches: ring kernel, any other
  uint64_t n_p2_roles = 0, n_p2_ring = 0, n_p2_sort = 0, n_p2_exact = 0, n_p1_ring = 0, n_p1_other = 0, n_tile_dense = 0, n_tile_nword = 0;
  // count --bc: the cache of admitted k-mers (kernels_bloom.hip.hpp) -- 0 undecided, 1 on, -1 off; decided from the first
  // filtered batches (host_partition.inl: bloom_cache_decide), dropped when the counter is detached
  DevBuf<uint64_t> d_bcache; int bcache_state = 0; uint64_t mers_seen = 0;
  uint64_t ovf_failed_need = 0;                  // the side-table size whose allocation failed (not retried per batch)
  bool returning = false;
  uint32_t out_counter_len = 4;
  // size doubling (hash_counter::do_size_doubling): occupancy bookkeeping, see ensure_capacity()
  bool grow_on = true;
  uint64_t occ_known = 0, fed_since = 0;
  uint64_t cur_bound = 0;        // the charge of the piece being ingested right now (launch_count -> part_ingest)
  uint64_t direct_seen = 0;      // CTR_DIRECT when the charges were last corrected
  uint64_t grow_seed = 0;
  // two-word keys (33 <= k <= 64): 128-bit slots, kernels_wide.hip.hpp
  bool wide = false;
  // keys of three or four words (65 <= k <= 128): 256-bit slots, kernels_nword.hip.hpp; partitioned path: kernels_nword_part.hip.hpp
  bool nword = false;
  NTable nt{};
  WideTable wt{};
  uint32_t key_words = 1;        // 64-bit words of a key in the API (mer_dna::data(): ceil(2k / 64))
  uint32_t slot_words = 1;       // 64-bit words of a table slot (1, 2 or 4)
  // staging for host buffers
  DevBuf<uint8_t> d_stage[2];
  Event stage_done[2];
  int stage_next = 0;
  // profiling
  bool prof_on = false;
  std::vector<ProfSpan> prof_pending;
  std::vector<Event> ev_all;         // every event of the profile spans, for good
  std::vector<hipEvent_t> ev_pool;   // ... and those of them that are free (get_event)
  std::vector<std::pair<int, float>> prof_log;   // every span since the last reset, in launch order (jfgpu_profile_spans)
  double prof_ms[kNumProf] = {};
  uint64_t prof_launches[kNumProf] = {};
  uint64_t prof_units[kNumProf] = {};
  // partitioned insert path (kernels_part.hip.hpp)
  int mode = MODE_AUTO;
  bool part_ok = false;          // geometry admits the partitioned path
  PartGeom pg{};
  bool item32 = false;
  bool item128 = false;          // two-word keys: 128-bit items (kernels_wide_part.hip.hpp)
  bool item256 = false;          // keys of three and four words: 256-bit items (kernels_nword_part.hip.hpp)
  bool pristine = true;          // table known all-zero: tile_insert may skip the tile read
  std::vector<PendingBatch> pending;
  uint64_t pending_bytes = 0;
  bool ref_matrix = false;       // default matrix family: the reference's (glibc random() stream kept in `glibc`)
  bool xs_matrix = false;        // the xor-shift family (gf2_xorshift_matrix): doublings stay in it
  GlibcRandom glibc;
  int (*spill_fn)(void*) = nullptr; void* spill_user = nullptr;     // jfgpu_set_spill
  int operation = 0;             // what count_ascii does with a k-mer: 0 add, 1 set (prime), 2 update_add (jfgpu_set_operation)
  Tuning tun;                    // the JFGPU_* switches as they were when the table was created (tuning.hpp)
  Event flush_ev[2], flush_done;   // with stream2
  double items_per_byte = 0;     // k-mers per sequence byte seen by the last flush (0: unknown yet)
  uint64_t reserved_input = 0;   // sequence bytes the caller announced (jfgpu_reserve): lets forced flushes be spaced evenly
  DevBuf<uint32_t> d_M1; int g1 = 0;
  DevBuf<uint64_t> d_strag2; DevBuf<uint32_t> d_strag2_n; uint32_t strag2_lists = 0;      // ... and of the ring P2, one per workgroup
  DevBuf<uint64_t> d_strag; DevBuf<uint32_t> d_strag_n;      // straggler lists of the ring P1 (kernels_p1ring.hip.hpp), one per workgroup
  DevBuf<uint32_t> d_M2; int g2 = 0;
  // workspace arena for pending batches and flush temporaries: bump-allocated, reset at flush,
  // grown geometrically (allocation of tens of GB costs ~100 ms, so never inside the hot path twice)
  DevBuf<uint8_t> ws; size_t ws_cap = 0, ws_used = 0;
  // dump state
  bool dump_open = false;
  uint64_t dump_lower = 0, dump_upper = 0;
  int dump_have_ovf = 0;
  std::vector<uint64_t> dump_prefix;  // per tile exclusive prefix, size n_tiles + 1
  uint64_t dump_tile_cursor = 0;
  DevBuf<uint8_t> d_dump; uint64_t dump_cap_records = 0;
  DevBuf<uint64_t> d_tile_off;
};

namespace {

int use(const jfgpu_table* t) {
  if(!t) return fail(JFGPU_E_INVALID, "null table");
  HIP_TRY(hipSetDevice(t->device));
  if(t->failed) return fail(t->failed, t->failed_msg + " (earlier; the table must be cleared)");
  return JFGPU_OK;
}

size_t slot_bytes_of(const jfgpu_table* t) { return t->g.slot32 ? 4 : 8 * (size_t)t->slot_words; }
uint64_t n_tiles_of(const jfgpu_table* t) { return 1ull << (t->g.lsize_l - t->g.tile_bits); }
// the filter attached to the table (count --bc, --bf-size), which lives in the view of its key width
DevBloom& table_bloom(jfgpu_table* t) { return t->nword ? t->nt.bloom : t->wide ? t->wt.bloom : t->dt.bloom; }
const DevBloom& table_bloom(const jfgpu_table* t) { return table_bloom(const_cast<jfgpu_table*>(t)); }

int grid_for(const jfgpu_table* t, uint64_t work_items) {
  uint64_t g = std::min<uint64_t>(work_items, (uint64_t)t->n_cu * 8);
  return (int)std::max<uint64_t>(g, 1);
}

hipEvent_t get_event(jfgpu_table* t) {
  if(!t->ev_pool.empty()) { hipEvent_t e = t->ev_pool.back(); t->ev_pool.pop_back(); return e; }
  t->ev_all.emplace_back();
  (void)t->ev_all.back().create();
  return t->ev_all.back();
}

struct ProfScope {  // records a HIP-event pair around a launch on the table's stream
  jfgpu_table* t; int which; uint64_t units; hipEvent_t a = nullptr, b = nullptr;
  ProfScope(jfgpu_table* t_, int w, uint64_t u) : t(t_), which(w), units(u) {
    if(t->prof_on) { a = get_event(t); b = get_event(t); hipEventRecord(a, t->stream); }
  }
  ~ProfScope() {
    if(t->prof_on) { hipEventRecord(b, t->stream); t->prof_pending.push_back({a, b, which, units}); }
  }
};

void prof_collect(jfgpu_table* t) {
  for(auto& s : t->prof_pending) {
    float ms = 0;
    hipEventSynchronize(s.b);
    if(hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) {
      t->prof_ms[s.which] += ms; t->prof_launches[s.which] += 1; t->prof_units[s.which] += s.units;
      if(t->prof_log.size() < (size_t)1 << 16) t->prof_log.emplace_back(s.which, ms);
    }
    t->ev_pool.push_back(s.a); t->ev_pool.push_back(s.b);
  }
  t->prof_pending.clear();
}

int read_counters(jfgpu_table* t, uint64_t* out /* CTR_COUNT */) {
  HIP_TRY(hipMemcpyAsync(out, t->dt.counters, sizeof(uint64_t) * CTR_COUNT, hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  return JFGPU_OK;
}

int check_deferred(jfgpu_table* t, uint64_t* ctr_out = nullptr) {
  uint64_t c[CTR_COUNT];
  int rc = read_counters(t, c);
  if(rc) return rc;
  if(ctr_out) memcpy(ctr_out, c, sizeof(c));
  if(c[CTR_MISROUTED])
    return fail(JFGPU_E_INVALID, std::to_string(c[CTR_MISROUTED]) + " k-mers were added to a shard that does not own them");
  if(c[CTR_FULL]) return fail(JFGPU_E_FULL, "Hash full");
  if(c[CTR_OVF_FULL]) return fail(JFGPU_E_FULL, "Hash full (count overflow table exhausted)");
  return JFGPU_OK;
}

bool use_partitioned(const jfgpu_table* t, size_t nbytes);
bool nword_auto_partitioned(const TableGeom& g, size_t nbytes);
int part_ingest(jfgpu_table* t, const uint8_t* base, int64_t lo, int64_t hi, bool from_keys, uint64_t max_items);
int part_flush(jfgpu_table* t);
int table_grow(jfgpu_table* t);
int measure_occupancy(jfgpu_table* t);
int comm_filter_ok(const jfgpu_table* t);   // abi_comm.inl

// Splits a device buffer pointer into a 16-byte aligned base and [lo, hi).
void align_buffer(const char* d, size_t n, const uint8_t*& base, int64_t& lo, int64_t& hi) {
  const uintptr_t p = (uintptr_t)d;
  const uintptr_t a = p & ~(uintptr_t)15;
  base = (const uint8_t*)a; lo = (int64_t)(p - a); hi = lo + (int64_t)n;
}

// ---- the overflow side table grows with what it may have to hold -------------------------------------------------
// A count field of cnt_bits bits wraps into the side table (ovf_add: one entry per key, units of 2^cnt_bits).  An entry
// costs its key 2^cnt_bits occurrences (or one add of a value that large), so (occurrences fed >> cnt_bits) + large adds
// bounds the entries whatever the input; the table is kept at twice that, rebuilt larger before the work that could
// fill it is enqueued (the 32-bit slots of round 2 brought count fields of 8-10 bits: a fixed-size side table then
// fails on repeat-rich input, where the reference just keeps counting: large_hash_array.hpp:887-937).
__global__ void ovf_rehash_kernel(const uint64_t* __restrict__ okey, const uint64_t* __restrict__ ocnt, uint64_t ocap,
                                  uint64_t* __restrict__ nkey, uint64_t* __restrict__ ncnt, uint64_t nmask, unsigned long long* __restrict__ lost) {
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ocap; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t want = okey[i];
    if(!want) continue;
    const uint64_t h = ((want - 1) * 0x9E3779B97F4A7C15ull) >> 20;
    bool placed = false;
    for(uint64_t p = 0; p <= nmask && !placed; ++p) {
      const uint64_t s = (h + p) & nmask;
      const unsigned long long old = atomicCAS((unsigned long long*)&nkey[s], 0ull, (unsigned long long)want);
      if(old == 0ull || old == want) { atomicAdd((unsigned long long*)&ncnt[s], (unsigned long long)ocnt[i]); placed = true; }
    }
    if(!placed) atomicAdd(lost, 1ull);
  }
}

// The two- and N-word views of the table share its slots, hash tables, side table and counters: what a view holds of them, from
// the DevTable (create, doubling, a side table rebuilt larger).  Geometry and filter are the view's own.
template <class View> void fill_view(View& v, const DevTable& d) {
  v.slots = d.slots; v.fwd_tbl = d.fwd_tbl; v.inv_tbl = d.inv_tbl; v.ovf_key = d.ovf_key; v.ovf_cnt = d.ovf_cnt;
  v.ovf_mask = d.ovf_mask; v.counters = d.counters; v.max_probe = d.max_probe;
  if constexpr(std::is_same_v<View, WideTable>) v.dirty = d.dirty;
}
void refresh_views(jfgpu_table* t);

int ensure_ovf(jfgpu_table* t, uint64_t more_occurrences, uint64_t more_big_adds) {
  t->occ_bound += more_occurrences; t->bigval_bound += more_big_adds;
  if(!t->returning) return JFGPU_OK;                              // count fields of 40 bits and more
  // entries are keyed by slot: there are never more of them than slots, whatever was fed (round-3 advisor finding: the
  // bound alone asked for 32 GB of side table at 100 Gbp into 10-bit count fields)
  const uint64_t slots = 1ull << t->g.lsize_l;
  const uint64_t need = std::min<uint64_t>(2 * ((t->occ_bound >> t->g.cnt_bits) + t->bigval_bound) + 4096, std::max<uint64_t>(2 * slots, 4096));
  if(need <= t->ovf_cap || need <= t->ovf_failed_need) return JFGPU_OK;      // (a size that could not be had is not asked for again until the table is cleared or grows)
  uint64_t cap2 = t->ovf_cap;
  while(cap2 < 2 * need && cap2 < 4 * slots) cap2 <<= 1;          // (room for the next few batches too)
  while(cap2 < need) cap2 <<= 1;
  HIP_TRY(hipStreamSynchronize(t->stream));
  if(t->stream2) HIP_TRY(hipStreamSynchronize(t->stream2));
  DevBuf<uint64_t> nk, nc;
  if(!nk.try_alloc(cap2) || !nc.try_alloc(cap2)) {
    (void)hipGetLastError();
    t->ovf_failed_need = need;
    return JFGPU_OK;                                              // no memory: carry on, CTR_OVF_FULL reports it if it really overflows
  }
  HIP_TRY(hipMemsetAsync(nk, 0, cap2 * 8, t->stream));
  HIP_TRY(hipMemsetAsync(nc, 0, cap2 * 8, t->stream));
  hipLaunchKernelGGL(ovf_rehash_kernel, dim3(grid_for(t, t->ovf_cap / kBlock + 1)), dim3(kBlock), 0, t->stream, t->dt.ovf_key, t->dt.ovf_cnt, t->ovf_cap, nk.get(), nc.get(), cap2 - 1,
                     (unsigned long long*)&t->dt.counters[CTR_OVF_FULL]);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(t->stream));
  t->ovf_key = std::move(nk); t->ovf_cnt = std::move(nc);
  t->dt.ovf_key = t->ovf_key; t->dt.ovf_cnt = t->ovf_cnt; t->dt.ovf_mask = cap2 - 1; t->ovf_cap = cap2;
  refresh_views(t);
  return JFGPU_OK;
}

int launch_count_chunk(jfgpu_table* t, const char* d_bases, size_t n);

// How many more k-mers may be enqueued before the table could exceed 80 % load, assuming every one
// of them is new (an upper bound: duplicates are only discovered by inserting).
uint64_t capacity_limit(const jfgpu_table* t) { return ((1ull << t->g.lsize_l) / 10) * 8; }
bool capacity_managed(const jfgpu_table* t) { return (t->grow_on || t->spill_fn) && t->g.shard_bits == 0 && t->g.lsize_g < t->g.key_bits && (!(t->wide || t->nword) || t->g.lsize_g < 48); }

// The size passed at creation is a hint (doc/Readme.md:67-72; hash_counter::handle_full_ary,
// hash_counter.hpp:178-198): before enqueuing `incoming` potential new keys make sure they cannot
// overflow the table -- measure the true occupancy when the running upper bound runs out, double the
// table (cooperative rehash on the device) when it is really more than half full.  Returns the
// number of k-mers that may be enqueued now (<= incoming, > 0).
extern "C" int jfgpu_clear(jfgpu_table* t);
int refine_pending_charges(jfgpu_table* t);
int ensure_capacity(jfgpu_table* t, uint64_t incoming, uint64_t* allowed) {
  *allowed = incoming;
  if(!capacity_managed(t)) return JFGPU_OK;
  uint64_t limit = capacity_limit(t);
  if(t->occ_known + t->fed_since + incoming <= limit) { t->fed_since += incoming; return JFGPU_OK; }
  // the charges are one k-mer per input byte; what is pending knows its exact item count (no flush needed to read it)
  int rc = refine_pending_charges(t); if(rc) return rc;
  if(t->occ_known + t->fed_since + incoming <= limit) { t->fed_since += incoming; return JFGPU_OK; }
  rc = measure_occupancy(t); if(rc) return rc;
  if(!t->grow_on) {
    // --disk (count_main.cc:276-277, hash_counter.hpp:178-198 with a dumper): when what is left would not take a
    // useful piece, the caller writes the table out as one sorted run, the table is emptied and counting goes on
    // (the runs are merged at the end).  Pieces never exceed the room left, so nothing is ever dropped.
    uint64_t room = limit > t->occ_known ? limit - t->occ_known : 0;
    if(room < std::min<uint64_t>(incoming, std::max<uint64_t>(limit / 8, 1))) {
      rc = check_deferred(t); if(rc) return rc;
      if(t->spill_fn(t->spill_user) != 0) return fail(JFGPU_E_INVALID, "the spill callback failed");
      rc = jfgpu_clear(t); if(rc) return rc;
      room = capacity_limit(t);
    }
    *allowed = std::max<uint64_t>(1, std::min<uint64_t>(incoming, room));
    t->fed_since += *allowed;
    return JFGPU_OK;
  }
  const uint64_t min_piece = std::min<uint64_t>(incoming, 65536);      // never enqueue less than this at a time
  while(true) {
    limit = capacity_limit(t);
    const uint64_t headroom = limit > t->occ_known ? limit - t->occ_known : 0;
    const bool really_full = t->occ_known > (1ull << t->g.lsize_l) / 2;
    if(!really_full && headroom >= min_piece) break;
    if(t->g.lsize_g >= t->g.key_bits) break;                             // 4^k positions: cannot fill up
    rc = table_grow(t);
    if(rc < 0) break;            // no memory for a bigger table: carry on, "Hash full" if it really overflows
    if(rc) return rc;
  }
  limit = capacity_limit(t);
  const uint64_t headroom = limit > t->occ_known ? limit - t->occ_known : 0;
  *allowed = std::min<uint64_t>(incoming, std::max<uint64_t>(headroom, min_piece));
  t->fed_since += *allowed;
  return JFGPU_OK;
}

int launch_count(jfgpu_table* t, const char* d_bases, size_t n) {
  if(n < t->g.k) return JFGPU_OK;
  if(!capacity_managed(t) || t->operation == 2) return launch_count_chunk(t, d_bases, n);   // an update pass adds no keys
  size_t off = 0;
  while(true) {
    uint64_t take = 0;
    int rc = ensure_capacity(t, n - off, &take); if(rc) return rc;
    // a piece holds at least one window and moves forward (spill mode may grant less than k characters of room; the few
    // extra k-mers cannot take the table past its 80 % bound by more than 2k)
    if(take < 2 * (uint64_t)t->g.k) take = std::min<uint64_t>(n - off, 2 * (uint64_t)t->g.k);
    t->cur_bound = take;
    rc = launch_count_chunk(t, d_bases + off, (size_t)take);
    t->cur_bound = 0;
    if(rc) return rc;
    if(off + take >= n) return JFGPU_OK;
    off += take - (t->g.k - 1);          // next piece re-reads the last k-1 characters: every window exactly once
  }
}

int ensure_stage(jfgpu_table* t) {
  for(int i = 0; i < 2; ++i) {
    int rc;
    if(!t->d_stage[i] && (rc = t->d_stage[i].alloc(kStageBytes))) return rc;
    if(!t->stage_done[i] && (rc = t->stage_done[i].create(hipEventDisableTiming))) return rc;
  }
  return JFGPU_OK;
}


#include "part_plan.inl"
#include "host_partition.inl"

// The view of the table for its key width (one, two, or three and four words), handed to a generic callable.
template <class F> void with_view(jfgpu_table* t, F&& f) {
  if(t->nword) f(t->nt); else if(t->wide) f(t->wt); else f(t->dt);
}

// One piece of sequence into the table: the partitioned path where it applies, else the direct kernel of the key width.
int launch_count_chunk(jfgpu_table* t, const char* d_bases, size_t n) {
  if(n < t->g.k) return JFGPU_OK;
  { int rc = ensure_ovf(t, n, 0); if(rc) return rc; }
  const uint8_t* base; int64_t lo, hi;
  align_buffer(d_bases, n, base, lo, hi);
  if(t->operation == 0 && use_partitioned(t, n)) {        // PRIME / UPDATE passes of --if run on the direct kernel
    const int rc = part_ingest(t, base, lo, hi, false, n);
    if(rc >= 0) return rc;          // < 0: batch too small for the single-pass partition / no memory for the pending batch -> direct kernel below
  }
  t->pristine = false;
  const dim3 grid(grid_for(t, (uint64_t)((hi + kTilePos - 1) / kTilePos))), block(kBlock);
  ProfScope ps(t, 0, n);
  with_view(t, [&](const auto& T) {
    typedef std::decay_t<decltype(T)> Table;
    with_flags(t->returning, T.bloom.data != nullptr, [&](auto RT, auto BL) {
      constexpr bool rt = decltype(RT)::value, bl = decltype(BL)::value;
      if constexpr(std::is_same_v<Table, NTable>) hipLaunchKernelGGL((count_ascii_nword_kernel<rt, bl>), grid, block, 0, t->stream, T, base, lo, hi, t->operation);
      else if constexpr(std::is_same_v<Table, WideTable>) hipLaunchKernelGGL(count_ascii_wide_kernel<rt>, grid, block, 0, t->stream, T, base, lo, hi, t->operation);   // (takes no BL flag)
      else hipLaunchKernelGGL((count_ascii_kernel<rt, bl>), grid, block, 0, t->stream, T, base, lo, hi, t->operation);
    });
  });
  HIP_TRY(hipGetLastError());
  return JFGPU_OK;
}

// stats / histo / tile counts / digest: the one-word kernels, scan_kernel for the wider keys.
// out: 64-bit counters, zeroed by the caller (tile_counts for SCAN_TILES: the wider keys want them zeroed as well).
struct ScanArgs { int what; uint64_t lower = 0, upper = ~0ull; int have_ovf = 0; uint64_t hbase = 0, hceil = 0, hinc = 1, nb = 1; };
void launch_scan(jfgpu_table* t, const DevTable& T, const ScanArgs& a, unsigned long long* out, uint32_t* tile_counts) {
  const dim3 grid(grid_for(t, (1ull << t->g.lsize_l) / kBlock + 1)), block(kBlock);
  if(a.what == SCAN_STATS) hipLaunchKernelGGL(stats_kernel, grid, block, 0, t->stream, T, a.lower, a.upper, a.have_ovf, out);
  else if(a.what == SCAN_HISTO) hipLaunchKernelGGL(histo_kernel, grid, block, 0, t->stream, T, a.hbase, a.hceil, a.hinc, a.nb, a.have_ovf, out);
  else if(a.what == SCAN_DIGEST) hipLaunchKernelGGL(digest_kernel, grid, block, 0, t->stream, T, a.lower, a.upper, a.have_ovf, out);
  else hipLaunchKernelGGL(tile_count_kernel, dim3(grid_for(t, n_tiles_of(t))), block, 0, t->stream, T, a.lower, a.upper, a.have_ovf, n_tiles_of(t), tile_counts);
}
template <class Table>
void launch_scan(jfgpu_table* t, const Table& T, const ScanArgs& a, unsigned long long* out, uint32_t* tile_counts) {
  hipLaunchKernelGGL(scan_kernel<Table>, dim3(grid_for(t, (1ull << t->g.lsize_l) / kBlock + 1)), dim3(kBlock), 0, t->stream, T, a.what, a.lower, a.upper, a.have_ovf,
                     a.hbase, a.hceil, a.hinc, a.nb, out, tile_counts);
}

// Pass 2 of the sorted dump (jfgpu_dump_next) for tiles [t0, t0 + ntile): records at d_tile_off, into d_dump.
int launch_dump(jfgpu_table* t, const DevTable& T, uint64_t t0, uint64_t ntile, uint32_t key_bytes) {
  const size_t lds = ((size_t)8 << t->g.tile_bits) + ((size_t)2 << t->g.tile_bits) + (size_t)t->g.nbytes * 2048;      // > 64 KiB at tiles of 2^13 slots
  return launch_lds(dump_tiles_kernel, dim3(grid_for(t, ntile)), dim3(kBlock), lds, t->stream, T, t->dump_lower,
                    t->dump_upper, t->dump_have_ovf, t0, ntile, (const uint64_t*)t->d_tile_off, t->d_dump.get(), key_bytes,
                    t->out_counter_len);
}
template <class Table>
int launch_dump(jfgpu_table* t, const Table& T, uint64_t t0, uint64_t ntile, uint32_t key_bytes) {
  const size_t lds = ((size_t)(8 * KeyOps<Table>::kSlotWords) << t->g.tile_bits) + ((size_t)2 << t->g.tile_bits);     // 16 or 32 bytes of slot, 2 of index
  return launch_lds(dump_tiles_words_kernel<Table>, dim3(grid_for(t, ntile)), dim3(kBlock), lds, t->stream, T, t->dump_lower, t->dump_upper,
                    t->dump_have_ovf, t0, ntile, (const uint64_t*)t->d_tile_off, t->d_dump.get(), key_bytes, t->out_counter_len);
}

// The sender's two passes over one contract buffer (route_count_kernel, route_scatter_kernel): the buffer's k-mers into `out`,
// grouped by owner, key_words words each.  d_cnt: one device counter per shard; counts[p]: the k-mers of owner p, whose
// region starts at counts[0] + .. + counts[p - 1] k-mers.  `capacity` is what `out` holds, in k-mers.  The host waits for the
// counts (one small copy) -- they place the regions -- and for the scatter.
int route_buffer(jfgpu_table* t, const char* d_bases, size_t n, unsigned long long* d_cnt, uint64_t* out, size_t capacity, uint64_t* counts) {
  const uint32_t W = 1u << t->g.shard_bits;
  const uint8_t* base; int64_t lo, hi;
  align_buffer(d_bases, n, base, lo, hi);
  const int grid = grid_for(t, (uint64_t)((hi + kTilePos - 1) / kTilePos));
  auto launch = [&](bool scatter) {
    ProfScope ps(t, 2, scatter ? 0 : n);
    int rc = JFGPU_OK;
    with_view(t, [&](const auto& T) {
      typedef std::decay_t<decltype(T)> Table;
      typedef KeyOps<Table> K;
      const size_t lds = K::kFwdLdsWords ? 0 : route_lds_bytes(t->g.nbytes, K::kHaloWords);
      auto go = [&](auto bloom) {
        if(scatter) rc = launch_lds(route_scatter_kernel<Table, decltype(bloom)::value>, dim3(grid), dim3(kBlock), lds, t->stream, T, base, lo, hi, d_cnt, out, t->key_words);
        else rc = launch_lds(route_count_kernel<Table, decltype(bloom)::value>, dim3(grid), dim3(kBlock), lds, t->stream, T, base, lo, hi, d_cnt);
      };
      if constexpr(std::is_same_v<Table, NTable>) go(std::false_type());      // (takes no filter)
      else if(T.bloom.data) go(std::true_type());
      else go(std::false_type());
    });
    return rc;
  };
  HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * W, t->stream));
  { const int rc = launch(false); if(rc) return rc; }
  std::vector<unsigned long long> h(W);
  HIP_TRY(hipMemcpyAsync(h.data(), d_cnt, sizeof(unsigned long long) * W, hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  uint64_t total = 0;
  for(uint32_t p = 0; p < W; ++p) { counts[p] = h[p]; h[p] = total; total += counts[p]; }
  if(total > capacity) return fail(JFGPU_E_INVALID, "partition buffer too small: need " + std::to_string(total) + " keys");
  HIP_TRY(hipMemcpyAsync(d_cnt, h.data(), sizeof(unsigned long long) * W, hipMemcpyHostToDevice, t->stream));   // cursors = offsets
  { const int rc = launch(true); if(rc) return rc; }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(t->stream));       // (the host vector h is read by the copy above)
  return JFGPU_OK;
}

// One scan into n 64-bit counters of its own (4, or a histogram's buckets), copied to `out` when it is complete.
int scan_to_host(jfgpu_table* t, const ScanArgs& a, uint64_t n, uint64_t* out) {
  DevBuf<unsigned long long> d;
  int rc = d.alloc(n); if(rc) return rc;
  HIP_TRY(hipMemsetAsync(d, 0, n * sizeof(unsigned long long), t->stream));
  with_view(t, [&](const auto& T) { launch_scan(t, T, a, d.get(), (uint32_t*)nullptr); });
  hipError_t e = hipMemcpyAsync(out, d, n * sizeof(uint64_t), hipMemcpyDeviceToHost, t->stream);
  if(e == hipSuccess) e = hipStreamSynchronize(t->stream);
  if(e != hipSuccess) return fail(JFGPU_E_HIP, hipGetErrorString(e));
  return JFGPU_OK;
}

int measure_occupancy(jfgpu_table* t) {
  int rc = part_flush(t); if(rc) return rc;
  uint64_t c[CTR_COUNT];
  rc = check_deferred(t, c); if(rc) return rc;
  uint64_t h[4];
  rc = scan_to_host(t, ScanArgs{SCAN_STATS}, 4, h); if(rc) return rc;
  t->occ_known = h[1]; t->fed_since = 0;
  return JFGPU_OK;
}

// Double the table: one more matrix row (so old positions are the low bits of new ones), new slots,
// rehash on the device, swap.  < 0: not possible (memory) -- the caller carries on with the old table.
// In three parts, because a SHARD grows together with the other shards of its table (abi_comm.inl: comm_grow): the new
// geometry, matrix and allocations (grow_prepare), what moves the entries (the rehash kernels here; a redistribution
// between the ranks there), and the exchange of old for new (grow_swap).
struct GrowNew {
  TableGeom g2; WideGeom w2; NGeom ng2;
  Gf2Matrix m2;
  DevTable nd; WideTable nw; NTable nn;
  DevBuf<uint8_t> slots, dirty;            // the new table's blocks until grow_swap hands them to the table; nd, nw and nn point at them
  DevBuf<uint64_t> ovf_key, ovf_cnt, nf, ni;
  uint64_t cap2 = 0;
  uint64_t ctr[CTR_COUNT];
  void drop() { slots = {}; dirty = {}; ovf_key = {}; ovf_cnt = {}; nf = {}; ni = {}; }      // a prepared doubling that will not happen
};
// ... and the old view together with the new one
template <class F> void with_view(jfgpu_table* t, GrowNew& N, F&& f) {
  if(t->nword) f(t->nt, N.nn); else if(t->wide) f(t->wt, N.nw); else f(t->dt, N.nd);
}

int grow_prepare(jfgpu_table* t, GrowNew& N) {
  int rc = part_flush(t); if(rc) return rc;
  rc = check_deferred(t, N.ctr); if(rc) return rc;
  const uint32_t r = t->g.lsize_g, c = t->g.key_bits;
  if(r >= c) return -1;
  Gf2Matrix& m2 = N.m2;
  m2 = t->matrix; m2.r = r + 1; m2.identity = false;
  std::vector<uint64_t> fwd, inv;
  if(t->xs_matrix) {
    m2 = gf2_xorshift_matrix(r + 1, c);
    if(!gf2_build_tables(m2, fwd, inv)) return fail(JFGPU_E_INVALID, "xor-shift matrix: singular low block");
  } else if(t->ref_matrix) {
    // like the reference: a brand-new matrix for the doubled table, next in the same random() stream
    for(int tries = 0; ; ++tries) {
      m2 = r + 1 >= c ? gf2_identity(r + 1, c) : gf2_reference_matrix(r + 1, c, t->glibc);
      if(gf2_build_tables(m2, fwd, inv)) break;
      if(tries > 1000) return fail(JFGPU_E_INVALID, "could not draw a hash matrix");
    }
  } else {
    // seeded family: extend the matrix by a random top row until the (r+1) x (r+1) low block is invertible again
    uint64_t st = (t->params.matrix_seed ? t->params.matrix_seed : kDefaultSeed) ^ (0xD6E8FEB86659FD93ull * (r + 1)) ^ t->grow_seed;
    for(int tries = 0; ; ++tries) {
      for(uint32_t j = 0; j < c; ++j) m2.columns[j] = (t->matrix.columns[j] & ((1ull << r) - 1)) | ((splitmix64(st) & 1ull) << r);
      if(gf2_build_tables(m2, fwd, inv)) break;
      if(tries > 1000) return fail(JFGPU_E_INVALID, "could not extend the hash matrix");
    }
  }
  TableGeom& g2 = N.g2;
  if(t->nword) { if(!nword_geom_init(N.ng2, t->g.k, r + 1, t->g.canonical, t->g.shard_bits, t->g.shard_id)) return -1; g2 = N.ng2.g; }
  else if(t->wide) { if(!wide_geom_init(N.w2, t->g.k, r + 1, t->g.canonical, t->g.shard_bits, t->g.shard_id)) return -1; g2 = N.w2.g; }
  else if(!geom_init(g2, t->g.k, r + 1, t->g.shard_bits, t->g.shard_id, t->g.canonical, !t->tun.slot64)) return -1;
  if(!t->nword) { g2.hash_xs = gf2_is_xorshift(m2) ? 1 : 0; if(t->wide) N.w2.g.hash_xs = g2.hash_xs; }
  const uint64_t n2 = 1ull << g2.lsize_l;
  const size_t slot_bytes = g2.slot32 ? 4 : 8 * (size_t)t->slot_words;
  uint64_t cap2 = std::max<uint64_t>(kMinOvf, std::min<uint64_t>(n2 / 256, 1ull << 26));
  if(g2.cnt_bits < 40) cap2 = std::max<uint64_t>(cap2, std::min<uint64_t>(2 * ((t->occ_bound >> g2.cnt_bits) + t->bigval_bound) + 4096, 2 * n2));      // (ensure_ovf's rule)
  cap2 = std::max<uint64_t>(cap2, t->ovf_cap);
  { uint64_t x = 1; while(x < cap2) x <<= 1; cap2 = x; }
  N.cap2 = cap2;
  DevTable& nd = N.nd;
  nd = t->dt;
  nd.g = g2; nd.slots = nullptr; nd.ovf_key = nd.ovf_cnt = nullptr; nd.dirty = nullptr;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if(n2 * slot_bytes + cap2 * 16 + ((size_t)1 << 30) > free_b) return -1;
  const bool ok = N.slots.try_alloc(n2 * slot_bytes) && N.ovf_key.try_alloc(cap2) && N.ovf_cnt.try_alloc(cap2) &&
                  N.dirty.try_alloc((size_t)1 << (g2.lsize_l - g2.tile_bits)) && N.nf.try_alloc(fwd.size()) && N.ni.try_alloc(inv.size());
  if(!ok) {
    N.drop();
    (void)hipGetLastError();
    return -1;
  }
  nd.slots = (decltype(nd.slots))N.slots.get(); nd.ovf_key = N.ovf_key; nd.ovf_cnt = N.ovf_cnt; nd.dirty = N.dirty;
  nd.fwd_tbl = N.nf; nd.inv_tbl = N.ni; nd.ovf_mask = cap2 - 1;
  nd.max_probe = (uint32_t)std::min<uint64_t>(g2.tile_mask, 1023);
  HIP_TRY(hipMemsetAsync(nd.slots, 0, n2 * slot_bytes, t->stream));
  HIP_TRY(hipMemsetAsync(nd.ovf_key, 0, cap2 * 8, t->stream));
  HIP_TRY(hipMemsetAsync(nd.ovf_cnt, 0, cap2 * 8, t->stream));
  HIP_TRY(hipMemsetAsync(nd.dirty, 0, (size_t)1 << (g2.lsize_l - g2.tile_bits), t->stream));
  HIP_TRY(hipMemcpyAsync(N.nf, fwd.data(), fwd.size() * 8, hipMemcpyHostToDevice, t->stream));
  HIP_TRY(hipMemcpyAsync(N.ni, inv.data(), inv.size() * 8, hipMemcpyHostToDevice, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));                  // (fwd / inv are this function's)
  N.nw = t->wt; N.nn = t->nt;
  if(t->nword) { N.nn.N = N.ng2; fill_view(N.nn, nd); }
  else if(t->wide) { N.nw.W = N.w2; fill_view(N.nw, nd); }
  return JFGPU_OK;
}

// the new table takes the old one's place (the entries have been moved and the stream is idle)
int grow_swap(jfgpu_table* t, GrowNew& N) {
  t->slots = std::move(N.slots); t->ovf_key = std::move(N.ovf_key); t->ovf_cnt = std::move(N.ovf_cnt); t->dirty = std::move(N.dirty);
  t->d_fwd = std::move(N.nf); t->d_inv = std::move(N.ni);
  t->dt = N.nd; t->g = N.g2; t->matrix = N.m2; t->ovf_cap = N.cap2;
  t->returning = t->g.cnt_bits < 40; t->ovf_failed_need = 0;
  (void)t->d_M2.reset();
  (void)t->d_strag.reset(); (void)t->d_strag_n.reset();     // (the item width may change with the geometry)
  if(t->nword) t->nt = N.nn;
  if(t->wide) t->wt = N.nw;
  part_geom_init(t);
  if(t->mode == MODE_PARTITIONED && !t->part_ok) t->mode = MODE_AUTO;
  t->pristine = false;
  ++t->grow_seed;
  return check_deferred(t);
}

int table_grow(jfgpu_table* t) {
  GrowNew N;
  int rc = grow_prepare(t, N); if(rc) return rc;
  const int have_ovf = (int)(N.ctr[CTR_OVF_USED] != 0);
  const dim3 grid(grid_for(t, (1ull << t->g.lsize_l) / kBlock + 1)), block(kBlock);
  with_view(t, N, [&](const auto& old, const auto& neu) { hipLaunchKernelGGL(rehash_kernel<std::decay_t<decltype(neu)>>, grid, block, 0, t->stream, old, neu, have_ovf); });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(t->stream));
  return grow_swap(t, N);
}

void refresh_views(jfgpu_table* t) {
  if(t->nword) fill_view(t->nt, t->dt);
  if(t->wide) fill_view(t->wt, t->dt);
}

bool use_partitioned(const jfgpu_table* t, size_t nbytes) {
  if(!t->part_ok || t->mode == MODE_DIRECT) return false;
  // keys of three and four words: a table with a filter attached and a shard stay on the direct kernel
  if(t->nword) return !t->nt.bloom.data && t->g.shard_bits == 0 && (t->mode == MODE_PARTITIONED || nword_auto_partitioned(t->g, nbytes));
  if(t->mode == MODE_PARTITIONED) return true;
  return nbytes >= kPartMinBytes || !t->pending.empty();
}

}  // namespace

extern "C" {

const char* jfgpu_last_error(void) { return g_err.c_str(); }
int jfgpu_abi_version(void) { return JFGPU_ABI_VERSION; }

int jfgpu_device_count(void) {
  int n = 0;
  if(hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int jfgpu_create(const jfgpu_params* p, jfgpu_table** out) {
  if(!p || !out) return fail(JFGPU_E_INVALID, "null argument");
  *out = nullptr;
  if(p->k < 1) return fail(JFGPU_E_INVALID, "mer length must be >= 1");
  if(p->k > 128) return fail(JFGPU_E_UNSUPPORTED, "mer length > 128 (more than four key words) is not built");
  if(p->shard_bits > 8) return fail(JFGPU_E_INVALID, "at most 256 shards");
  if(p->shard_id >= (1u << p->shard_bits)) return fail(JFGPU_E_INVALID, "shard_id out of range");
  int dev = 0;
  int rc = pick_device(p->device, &dev); if(rc) return rc;

  // size -> lsize (large_hash_array.hpp:156-157 rounds up to a power of two, :997-1000 caps at 4^k)
  const bool nword = p->k > 64, wide = p->k > 32 && !nword;
  uint32_t lsize = 0;
  while(lsize < 63 && (1ull << lsize) < p->size) ++lsize;
  if(nword) {
    lsize = std::max(lsize, nword_min_lsize(p->k));
    lsize = std::max<uint32_t>(lsize, kNTileBits + p->shard_bits);        // a shard holds at least one tile
    lsize = std::min<uint32_t>(lsize, 48);
  } else if(wide) {
    lsize = std::max(lsize, wide_min_lsize(p->k));
    lsize = std::max<uint32_t>(lsize, kMaxTileBits + p->shard_bits);       // a shard holds at least one tile
    lsize = std::min<uint32_t>(lsize, 48);
  } else {
    lsize = std::max(lsize, geom_min_lsize(p->k, p->shard_bits));
    lsize = std::max(lsize, p->shard_bits);
    lsize = std::max<uint32_t>(lsize, 1);
    lsize = std::min<uint32_t>(lsize, 2 * p->k);
    if(lsize < p->shard_bits) return fail(JFGPU_E_INVALID, "more shards than 4^k table positions");
  }

  std::unique_ptr<jfgpu_table> t(new jfgpu_table);
  t->tun = Tuning::from_env();
  t->tun.p2_cap = t->tun.p2_cap / kGran * kGran;
  t->params = *p; t->params.matrix_columns = nullptr;
  t->device = dev;
  t->out_counter_len = p->out_counter_len ? p->out_counter_len : 4;
  if(t->out_counter_len > 8) return fail(JFGPU_E_INVALID, "out_counter_len must be <= 8");
  t->wide = wide; t->nword = nword; t->key_words = (2 * p->k + 63) / 64; t->slot_words = nword ? kNWords : wide ? 2 : 1;
  if(nword) {
    if(!nword_geom_init(t->nt.N, p->k, lsize, p->canonical ? 1 : 0, p->shard_bits, p->shard_id)) return fail(JFGPU_E_INVALID, "table geometry does not fit a 256-bit slot");
    t->g = t->nt.N.g;
  } else if(wide) {
    if(!wide_geom_init(t->wt.W, p->k, lsize, p->canonical ? 1 : 0, p->shard_bits, p->shard_id)) return fail(JFGPU_E_INVALID, "table geometry does not fit a 128-bit slot");
    t->g = t->wt.W.g;
  } else if(!geom_init(t->g, p->k, lsize, p->shard_bits, p->shard_id, p->canonical ? 1 : 0, !t->tun.slot64))
    return fail(JFGPU_E_INVALID, "table geometry does not fit a 64-bit slot");

  // hash matrix (large_hash_array.hpp:992-1001)
  if(p->matrix_columns) {
    t->matrix.r = lsize; t->matrix.c = 2 * p->k;
    t->matrix.columns.assign(p->matrix_columns, p->matrix_columns + 2 * p->k);
    t->matrix.identity = gf2_is_low_identity(t->matrix);
  } else if(p->matrix_seed) {
    t->matrix = gf2_random(lsize, 2 * p->k, p->matrix_seed);
  } else if(p->k <= 64 && lsize < 2 * p->k && (p->matrix_kind ? p->matrix_kind : (uint32_t)t->tun.matrix) == JFGPU_MATRIX_XORSHIFT) {
    t->xs_matrix = true;
    t->matrix = gf2_xorshift_matrix(lsize, 2 * p->k);
  } else {
    // the reference's default: first matrix of an unseeded glibc random() stream; the stream stays with the
    // table so that doublings draw their matrices like hash_counter::double_size does (hash_counter.hpp:210-214)
    t->ref_matrix = true;
    t->matrix = lsize >= 2 * p->k ? gf2_identity(lsize, 2 * p->k) : gf2_reference_matrix(lsize, 2 * p->k, t->glibc);
  }
  if(!nword) {                                                                 // (also a matrix given by its columns: a file header's)
    t->g.hash_xs = gf2_is_xorshift(t->matrix) ? 1 : 0;
    if(wide) t->wt.W.g.hash_xs = t->g.hash_xs;
  }
  std::vector<uint64_t> fwd, inv;
  while(!gf2_build_tables(t->matrix, fwd, inv)) {
    if(!t->ref_matrix || t->matrix.identity) return fail(JFGPU_E_INVALID, "hash matrix: low r x r block is singular");
    t->matrix = gf2_reference_matrix(lsize, 2 * p->k, t->glibc);        // cannot happen for a pseudo-inverse; belt and braces
  }

  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  t->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  rc = t->stream.create(); if(rc) return rc;

  const uint64_t n_slots = 1ull << t->g.lsize_l;
  t->ovf_cap = std::max<uint64_t>(kMinOvf, std::min<uint64_t>(n_slots / 256, 1ull << 26));
  { uint64_t c = 1; while(c < t->ovf_cap) c <<= 1; t->ovf_cap = c; }
  t->returning = t->g.cnt_bits < 40;

  DevTable& d = t->dt;
  d.g = t->g;
  if((rc = t->slots.alloc(n_slots * slot_bytes_of(t.get()))) || (rc = t->d_fwd.alloc(fwd.size())) || (rc = t->d_inv.alloc(inv.size())) ||
     (rc = t->ovf_key.alloc(t->ovf_cap)) || (rc = t->ovf_cnt.alloc(t->ovf_cap)) || (rc = t->counters.alloc(CTR_COUNT)) ||
     (rc = t->dirty.alloc((size_t)1 << (t->g.lsize_l - t->g.tile_bits)))) return rc;
  d.slots = (decltype(d.slots))t->slots.get(); d.ovf_key = t->ovf_key; d.ovf_cnt = t->ovf_cnt; d.counters = (decltype(d.counters))t->counters.get(); d.dirty = t->dirty;
  d.fwd_tbl = t->d_fwd; d.inv_tbl = t->d_inv; d.ovf_mask = t->ovf_cap - 1;
  // Give up on a tile after 1024 probes (load > 99.8%); the reference gives up after 126
  // (count_main_cmdline.yaggo -p).  Small tiles are probed exhaustively.
  d.max_probe = (uint32_t)std::min<uint64_t>(t->g.tile_mask, 1023);
  HIP_TRY(hipMemcpy(t->d_fwd, fwd.data(), fwd.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t->d_inv, inv.data(), inv.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  if(nword) { fill_view(t->nt, d); memset(&t->nt.bloom, 0, sizeof t->nt.bloom); }
  else if(wide) { fill_view(t->wt, d); memset(&t->wt.bloom, 0, sizeof t->wt.bloom); }
  part_geom_init(t.get());
  if(t->tun.mode == 1) t->mode = MODE_DIRECT;
  else if(t->tun.mode == 2 && t->part_ok) t->mode = MODE_PARTITIONED;
  rc = jfgpu_clear(t.get());
  if(rc) { t->stream.sync(); return rc; }      // (drained before the handle goes, like every destroy path)
  *out = t.release();
  return JFGPU_OK;
}

void jfgpu_destroy(jfgpu_table* t) {
  if(!t) return;
  hipSetDevice(t->device);
  if(t->stream) hipStreamSynchronize(t->stream);
  prof_collect(t);
  part_discard(t);
  t->stream2.sync();
  delete t;
}

int jfgpu_get_info(const jfgpu_table* t, jfgpu_info* o) {
  if(!t || !o) return fail(JFGPU_E_INVALID, "null argument");
  memset(o, 0, sizeof(*o));
  o->k = t->g.k; o->key_len = t->g.key_bits; o->canonical = t->g.canonical;
  o->lsize = t->g.lsize_g; o->size = 1ull << t->g.lsize_g; o->local_size = 1ull << t->g.lsize_l;
  o->shard_bits = t->g.shard_bits; o->shard_id = t->g.shard_id;
  o->val_len = t->g.cnt_bits; o->slot_bytes = (uint32_t)slot_bytes_of(t); o->tile_slots = 1u << t->g.tile_bits;
  o->matrix_identity = t->matrix.identity ? 1 : 0;
  o->out_counter_len = t->out_counter_len;
  o->max_reprobe = t->dt.max_probe;
  o->table_bytes = (1ull << t->g.lsize_l) * slot_bytes_of(t);
  return JFGPU_OK;
}

int jfgpu_get_matrix(const jfgpu_table* t, uint64_t* columns) {
  if(!t || !columns) return fail(JFGPU_E_INVALID, "null argument");
  memcpy(columns, t->matrix.columns.data(), sizeof(uint64_t) * t->matrix.c);
  return JFGPU_OK;
}

int jfgpu_clear(jfgpu_table* t) {
  if(t) { t->failed = 0; t->failed_msg.clear(); }              // (what a failed flush left behind goes with everything else)
  int rc = use(t); if(rc) return rc;
  part_discard(t);
  HIP_TRY(hipMemsetAsync(t->dt.slots, 0, (1ull << t->g.lsize_l) * slot_bytes_of(t), t->stream));
  HIP_TRY(hipMemsetAsync(t->dt.ovf_key, 0, t->ovf_cap * sizeof(uint64_t), t->stream));
  HIP_TRY(hipMemsetAsync(t->dt.ovf_cnt, 0, t->ovf_cap * sizeof(uint64_t), t->stream));
  HIP_TRY(hipMemsetAsync(t->dt.counters, 0, CTR_COUNT * sizeof(uint64_t), t->stream));
  HIP_TRY(hipMemsetAsync(t->dt.dirty, 0, (size_t)1 << (t->g.lsize_l - t->g.tile_bits), t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  t->pristine = true; t->occ_known = 0; t->fed_since = 0; t->direct_seen = 0; t->occ_bound = 0; t->bigval_bound = 0; t->ovf_failed_need = 0;
  t->flushes_plain = 0; t->flushes_heavy = 0;
  t->n_p2_roles = t->n_p2_ring = t->n_p2_sort = t->n_p2_exact = t->n_p1_ring = t->n_p1_other = t->n_tile_dense = t->n_tile_nword = 0;
  return JFGPU_OK;
}

int jfgpu_sync(jfgpu_table* t) {
  int rc = use(t); if(rc) return rc;
  rc = part_flush(t); if(rc) return rc;
  HIP_TRY(hipStreamSynchronize(t->stream));
#ifdef JFGPU_PHASE_PROF
  { unsigned long long c[24], z[24] = {0};
    if(hipMemcpyFromSymbol(c, HIP_SYMBOL(g_phase_prof), sizeof c) == hipSuccess) {
      fprintf(stderr, "[phase prof] P1 (ring): stage %llu  encode+hash+append %llu  (barrier) %llu  units out %llu  finish %llu\n",
              c[0], c[1], c[2], c[3], c[4]);
      fprintf(stderr, "[phase prof] P2: (barrier) %llu  load %llu  hist %llu  scan %llu  lds-scatter %llu  write-out %llu  finish %llu\n",
              c[8], c[9], c[10], c[11], c[12], c[13], c[14]);
      fprintf(stderr, "[phase prof] T: loop+offsets %llu  rank adds + fill %llu  place %llu  merge %llu  queue (wave 0's own) %llu  (its wait for the others) %llu  store %llu\n",
              c[16], c[17], c[18], c[22], c[21], c[19], c[20]);
      (void)hipMemcpyToSymbol(HIP_SYMBOL(g_phase_prof), z, sizeof z);
    } }
#endif
#ifdef JFGPU_TILE_PROF
  { uint64_t c[CTR_COUNT]; if(read_counters(t, c) == JFGPU_OK)
      fprintf(stderr, "[tile prof] wait+prefetch %llu  fill %llu  insert %llu  store %llu (shader clocks, summed over blocks)\n",
              (unsigned long long)c[CTR_PROF0], (unsigned long long)c[CTR_PROF0 + 1], (unsigned long long)c[CTR_PROF0 + 2], (unsigned long long)c[CTR_PROF0 + 3]); }
#endif
  return check_deferred(t);
}

int jfgpu_wait(jfgpu_table* t) {
  int rc = use(t); if(rc) return rc;
  HIP_TRY(hipStreamSynchronize(t->stream));
  return JFGPU_OK;
}

int jfgpu_count_ascii_dev(jfgpu_table* t, const char* d_bases, size_t n) {
  int rc = use(t); if(rc) return rc;
  if(t->g.shard_bits) return fail(JFGPU_E_INVALID, "sharded table: count through its communicator (jfgpu_comm_count_ascii_dev)");
  if(!d_bases && n) return fail(JFGPU_E_INVALID, "null buffer");
  return launch_count(t, d_bases, n);
}

int jfgpu_count_ascii(jfgpu_table* t, const char* bases, size_t n) {
  int rc = use(t); if(rc) return rc;
  if(t->g.shard_bits) return fail(JFGPU_E_INVALID, "sharded table: count through its communicator (jfgpu_comm_count_ascii_dev)");
  if(!bases && n) return fail(JFGPU_E_INVALID, "null buffer");
  if(n < t->g.k) return JFGPU_OK;
  rc = ensure_stage(t); if(rc) return rc;
  // Chunks overlap by k-1 bytes so that every window is seen exactly once (the same
  // "seam" idea as mer_overlap_sequence_parser.hpp:164-167,182-184).
  const size_t step = kStageBytes - (t->g.k - 1);
  for(size_t o = 0; o < n; o += step) {
    const size_t len = std::min(kStageBytes, n - o);
    const int b = t->stage_next; t->stage_next ^= 1;
    HIP_TRY(hipEventSynchronize(t->stage_done[b]));  // kernel that last read this buffer has finished
    HIP_TRY(hipMemcpyAsync(t->d_stage[b], bases + o, len, hipMemcpyHostToDevice, t->stream));
    rc = launch_count(t, (const char*)t->d_stage[b].get(), len); if(rc) return rc;
    HIP_TRY(hipEventRecord(t->stage_done[b], t->stream));
    if(o + len >= n) break;
  }
  return JFGPU_OK;
}

// One piece of an add_keys batch that is known to fit (the capacity check was made by the caller).
static int add_keys_piece(jfgpu_table* t, const uint64_t* d_keys, size_t n, uint64_t val, uint8_t* d_is_new) {
  int rc = JFGPU_OK;
  if(!n) return JFGPU_OK;
  { const bool big = t->g.cnt_bits < 64 && (val >> t->g.cnt_bits) != 0;
    rc = ensure_ovf(t, big ? 0 : (uint64_t)n * val, big ? n : 0); if(rc) return rc; }
  // the partitioned path and its pending batch take keys of one word only
  const bool one_word = !t->wide && !t->nword;
  if(one_word && val == 1 && !d_is_new && use_partitioned(t, n * 8)) {
    const int prc = part_ingest(t, (const uint8_t*)d_keys, 0, (int64_t)n, true, n);
    if(prc >= 0) return prc;
  }
  if((one_word && (d_is_new || val != 1)) || t->nword) { rc = part_flush(t); if(rc) return rc; }   // is_new / set() must see earlier adds
  if(!t->wide) t->pristine = false;                      // (an add of two-word keys never cleared it: kept so)
  const int grid = grid_for(t, (n + kBlock - 1) / kBlock);
  ProfScope ps(t, 1, n);
  if(one_word && val == 1 && !d_is_new) {
    if(t->returning) hipLaunchKernelGGL(add_keys_one_kernel<true>, dim3(grid), dim3(kBlock), 0, t->stream, t->dt, d_keys, (uint64_t)n);
    else             hipLaunchKernelGGL(add_keys_one_kernel<false>, dim3(grid), dim3(kBlock), 0, t->stream, t->dt, d_keys, (uint64_t)n);
  } else {
    with_view(t, [&](const auto& T) {
      hipLaunchKernelGGL(add_keys_kernel<std::decay_t<decltype(T)>>, dim3(grid), dim3(kBlock), 0, t->stream, T, d_keys, (uint64_t)n, t->key_words, val, d_is_new);
    });
  }
  HIP_TRY(hipGetLastError());
  return JFGPU_OK;
}

int jfgpu_add_keys_dev(jfgpu_table* t, const uint64_t* d_keys, size_t n, uint64_t val, uint8_t* d_is_new) {
  int rc = use(t); if(rc) return rc;
  if(!n) return JFGPU_OK;
  if(!d_keys) return fail(JFGPU_E_INVALID, "null keys");
  if(!capacity_managed(t)) return add_keys_piece(t, d_keys, n, val, d_is_new);
  // In order, piece by piece: each piece is enqueued before the occupancy is looked at again, so a batch several
  // times the table's size doubles (or spills) the table as often as it has to (hash_counter::add, hash_counter.hpp:91-115)
  size_t off = 0;
  while(off < n) {
    uint64_t take = 0;
    rc = ensure_capacity(t, n - off, &take); if(rc) return rc;
    rc = add_keys_piece(t, d_keys + off * t->key_words, (size_t)take, val, d_is_new ? d_is_new + off : nullptr); if(rc) return rc;
    off += (size_t)take;
  }
  return JFGPU_OK;
}

int jfgpu_add_keys(jfgpu_table* t, const uint64_t* keys, size_t n, uint64_t val, uint8_t* is_new) {
  int rc = use(t); if(rc) return rc;
  if(!n) return JFGPU_OK;
  DevBuf<uint64_t> d_k; DevBuf<uint8_t> d_n;
  rc = d_k.alloc(n * t->key_words); if(rc) return rc;
  if(is_new && !d_n.try_alloc(n)) return fail(JFGPU_E_ALLOC, "hipMalloc is_new");
  hipError_t e = hipMemcpyAsync(d_k, keys, n * sizeof(uint64_t) * t->key_words, hipMemcpyHostToDevice, t->stream);
  if(e == hipSuccess) { rc = jfgpu_add_keys_dev(t, d_k, n, val, d_n); }
  if(e == hipSuccess && !rc && is_new) e = hipMemcpyAsync(is_new, d_n, n, hipMemcpyDeviceToHost, t->stream);
  hipStreamSynchronize(t->stream);
  if(e != hipSuccess) return fail(JFGPU_E_HIP, hipGetErrorString(e));
  if(rc) return rc;
  return check_deferred(t);
}

// hash_counter::add(key, val) for a batch with one value per key (large_hash_array.hpp:741-752 add_val with an arbitrary
// increment): what loads a binary/sorted file back into a table -- `query -s` answers from the device that way
// (sub_commands/query_main.cc:44-51).  Host arrays, staged; the growth / spill rules of jfgpu_add_keys.
int jfgpu_add_key_vals(jfgpu_table* t, const uint64_t* keys, const uint64_t* vals, size_t n) {
  int rc = use(t); if(rc) return rc;
  if(!n) return JFGPU_OK;
  if(!keys || !vals) return fail(JFGPU_E_INVALID, "null argument");
  if(t->g.shard_bits) return fail(JFGPU_E_UNSUPPORTED, "add_key_vals: not for a shard (route the keys first)");
  const size_t kw = t->key_words;
  DevBuf<uint64_t> d_k, d_v;
  rc = d_k.alloc(n * kw); if(rc) return rc;
  if(!d_v.try_alloc(n)) return fail(JFGPU_E_ALLOC, "hipMalloc values");
  auto done = [&](int r) { hipStreamSynchronize(t->stream); return r; };
  if(hipMemcpyAsync(d_k, keys, n * kw * sizeof(uint64_t), hipMemcpyHostToDevice, t->stream) != hipSuccess ||
     hipMemcpyAsync(d_v, vals, n * sizeof(uint64_t), hipMemcpyHostToDevice, t->stream) != hipSuccess) return done(fail(JFGPU_E_HIP, "add_key_vals: copy"));
  size_t off = 0;
  while(off < n) {
    uint64_t take = n - off;
    if(capacity_managed(t)) { rc = ensure_capacity(t, n - off, &take); if(rc) return done(rc); }
    uint64_t small = 0, big = 0;                              // what the overflow side table has to be ready for (ensure_ovf's two bounds)
    for(size_t i = off; i < off + take; ++i) { if(t->g.cnt_bits < 64 && (vals[i] >> t->g.cnt_bits)) ++big; else small += vals[i]; }
    rc = ensure_ovf(t, small, big); if(rc) return done(rc);
    rc = part_flush(t); if(rc) return done(rc);
    t->pristine = false;
    const dim3 grid(grid_for(t, take / kBlock + 1)), block(kBlock);
    with_view(t, [&](const auto& T) {
      hipLaunchKernelGGL(add_pairs_kernel<std::decay_t<decltype(T)>>, grid, block, 0, t->stream, T, (const uint64_t*)(d_k + off * kw), (const uint64_t*)(d_v + off), (uint64_t)take, t->key_words);
    });
    if(hipGetLastError() != hipSuccess) return done(fail(JFGPU_E_HIP, "add_key_vals: launch"));
    off += (size_t)take;
  }
  rc = done(JFGPU_OK);
  return rc ? rc : check_deferred(t);
}

int jfgpu_lookup_dev(jfgpu_table* t, const uint64_t* d_keys, size_t n, uint64_t* d_vals, uint8_t* d_found) {
  int rc = use(t); if(rc) return rc;
  rc = part_flush(t); if(rc) return rc;
  if(!n) return JFGPU_OK;
  if(!d_keys || !d_vals) return fail(JFGPU_E_INVALID, "null argument");
  uint64_t c[CTR_COUNT];
  rc = check_deferred(t, c); if(rc) return rc;
  const int grid = grid_for(t, (n + kBlock - 1) / kBlock);
  ProfScope ps(t, 3, n);
  with_view(t, [&](const auto& T) {
    hipLaunchKernelGGL(lookup_kernel<std::decay_t<decltype(T)>>, dim3(grid), dim3(kBlock), 0, t->stream, T, d_keys, (uint64_t)n, t->key_words, d_vals, d_found, (int)(c[CTR_OVF_USED] != 0));
  });
  HIP_TRY(hipGetLastError());
  return JFGPU_OK;
}

int jfgpu_lookup(jfgpu_table* t, const uint64_t* keys, size_t n, uint64_t* vals, uint8_t* found) {
  int rc = use(t); if(rc) return rc;
  if(!n) return JFGPU_OK;
  DevBuf<uint64_t> d_k, d_v; DevBuf<uint8_t> d_f;
  rc = d_k.alloc(n * t->key_words); if(rc) return rc;
  if(!d_v.try_alloc(n) || !d_f.try_alloc(n)) return fail(JFGPU_E_ALLOC, "hipMalloc lookup buffers");
  hipError_t e = hipMemcpyAsync(d_k, keys, n * sizeof(uint64_t) * t->key_words, hipMemcpyHostToDevice, t->stream);
  if(e == hipSuccess) rc = jfgpu_lookup_dev(t, d_k, n, d_v, d_f);
  if(e == hipSuccess && !rc) e = hipMemcpyAsync(vals, d_v, n * sizeof(uint64_t), hipMemcpyDeviceToHost, t->stream);
  if(e == hipSuccess && !rc && found) e = hipMemcpyAsync(found, d_f, n, hipMemcpyDeviceToHost, t->stream);
  hipStreamSynchronize(t->stream);
  if(e != hipSuccess) return fail(JFGPU_E_HIP, hipGetErrorString(e));
  return rc;
}

// query_from_sequence (query_main.cc:44-51) over one contract buffer: query_ascii_kernel
int jfgpu_query_ascii_dev(jfgpu_table* t, const char* d_bases, size_t n, uint64_t* d_vals, uint8_t* d_flags) {
  int rc = use(t); if(rc) return rc;
  rc = part_flush(t); if(rc) return rc;
  if(!n) return JFGPU_OK;
  if(!d_bases || !d_vals) return fail(JFGPU_E_INVALID, "null argument");
  if(t->g.shard_bits) return fail(JFGPU_E_UNSUPPORTED, "query_ascii: not for a shard (the keys of the other shards are not here)");
  uint64_t c[CTR_COUNT];
  rc = check_deferred(t, c); if(rc) return rc;
  const uint8_t* base; int64_t lo, hi;
  align_buffer(d_bases, n, base, lo, hi);
  const int grid = grid_for(t, (uint64_t)((hi + kTilePos - 1) / kTilePos));
  ProfScope ps(t, 8, n);
  with_view(t, [&](const auto& T) {
    typedef std::decay_t<decltype(T)> Table;
    typedef KeyOps<Table> K;
    const size_t lds = K::kFwdLdsWords ? 0 : query_lds_bytes(t->g.nbytes, K::kHaloWords);
    rc = launch_lds(query_ascii_kernel<Table>, dim3(grid), dim3(kBlock), lds, t->stream, T, base, lo, hi, d_vals, d_flags, (int)(c[CTR_OVF_USED] != 0));
  });
  if(rc) return rc;
  HIP_TRY(hipGetLastError());
  return JFGPU_OK;
}

// Host arrays, staged through the table's double buffer like jfgpu_count_ascii: pieces overlap by k - 1 bytes, and the
// first k - 1 outputs of every piece after the first (windows the piece before has answered, or that it alone sees
// whole) are not copied back.  The outputs of a piece are copied straight into the caller's arrays.
int jfgpu_query_ascii(jfgpu_table* t, const char* bases, size_t n, uint64_t* vals, uint8_t* flags) {
  int rc = use(t); if(rc) return rc;
  if(!n) return JFGPU_OK;
  if(!bases || !vals) return fail(JFGPU_E_INVALID, "null argument");
  if(t->g.shard_bits) return fail(JFGPU_E_UNSUPPORTED, "query_ascii: not for a shard (the keys of the other shards are not here)");
  rc = ensure_stage(t); if(rc) return rc;
  const size_t piece = std::min(kStageBytes, n), seam = t->g.k - 1;
  DevBuf<uint64_t> d_v; DevBuf<uint8_t> d_f;
  rc = d_v.alloc(piece); if(rc) return rc;
  if(flags && !d_f.try_alloc(piece)) return fail(JFGPU_E_ALLOC, "hipMalloc query flags");
  hipError_t e = hipSuccess;
  for(size_t o = 0; o < n && e == hipSuccess && !rc; o += kStageBytes - seam) {
    const size_t len = std::min(kStageBytes, n - o), skip = o ? seam : 0;
    const int b = t->stage_next; t->stage_next ^= 1;
    e = hipEventSynchronize(t->stage_done[b]);                 // the kernel that last read this buffer has finished
    if(e == hipSuccess) e = hipMemcpyAsync(t->d_stage[b], bases + o, len, hipMemcpyHostToDevice, t->stream);
    if(e == hipSuccess) rc = jfgpu_query_ascii_dev(t, (const char*)t->d_stage[b].get(), len, d_v, d_f);
    if(e == hipSuccess && !rc) e = hipEventRecord(t->stage_done[b], t->stream);
    if(e == hipSuccess && !rc) e = hipMemcpyAsync(vals + o + skip, d_v + skip, (len - skip) * sizeof(uint64_t), hipMemcpyDeviceToHost, t->stream);
    if(e == hipSuccess && !rc && flags) e = hipMemcpyAsync(flags + o + skip, d_f + skip, len - skip, hipMemcpyDeviceToHost, t->stream);
    if(e == hipSuccess && !rc) e = hipStreamSynchronize(t->stream);      // (d_v and d_f are the next piece's too)
    if(o + len >= n) break;
  }
  hipStreamSynchronize(t->stream);
  if(e != hipSuccess) return fail(JFGPU_E_HIP, hipGetErrorString(e));
  return rc;
}

int jfgpu_partition_ascii_dev(jfgpu_table* t, const char* d_bases, size_t n, uint64_t* d_keys_out, size_t capacity,
                              uint64_t* counts_out) {
  int rc = use(t); if(rc) return rc;
  if(!counts_out) return fail(JFGPU_E_INVALID, "null counts_out");
  rc = comm_filter_ok(t); if(rc) return rc;     // a one-pass filter changes as it is asked, and the two passes ask twice
  const uint32_t n_shards = 1u << t->g.shard_bits;
  for(uint32_t i = 0; i < n_shards; ++i) counts_out[i] = 0;
  if(n < t->g.k) return JFGPU_OK;
  if(!d_bases || !d_keys_out) return fail(JFGPU_E_INVALID, "null buffer");
  DevBuf<unsigned long long> d_cnt;
  rc = d_cnt.alloc(n_shards); if(rc) return rc;
  return route_buffer(t, d_bases, n, d_cnt, d_keys_out, capacity, counts_out);
}

int jfgpu_stats_compute(jfgpu_table* t, uint64_t lower, uint64_t upper, jfgpu_stats* out) {
  int rc = use(t); if(rc) return rc;
  rc = part_flush(t); if(rc) return rc;
  if(!out) return fail(JFGPU_E_INVALID, "null out");
  uint64_t c[CTR_COUNT];
  rc = check_deferred(t, c); if(rc) return rc;
  uint64_t h[4];
  rc = scan_to_host(t, ScanArgs{SCAN_STATS, lower, upper, (int)(c[CTR_OVF_USED] != 0)}, 4, h); if(rc) return rc;
  out->unique = h[0]; out->distinct = h[1]; out->total = h[2]; out->max_count = h[3];
  out->occupied = h[1]; out->mers_fed = c[CTR_MERS];
  return JFGPU_OK;
}

int jfgpu_digest(jfgpu_table* t, uint64_t lower, uint64_t upper, uint64_t* out4) {
  int rc = use(t); if(rc) return rc;
  rc = part_flush(t); if(rc) return rc;
  if(!out4) return fail(JFGPU_E_INVALID, "null out");
  uint64_t c[CTR_COUNT];
  rc = check_deferred(t, c); if(rc) return rc;
  return scan_to_host(t, ScanArgs{SCAN_DIGEST, lower, upper, (int)(c[CTR_OVF_USED] != 0)}, 4, out4);
}

int jfgpu_histo(jfgpu_table* t, uint64_t base, uint64_t ceil, uint64_t inc, uint64_t* histo, uint64_t nb) {
  int rc = use(t); if(rc) return rc;
  rc = part_flush(t); if(rc) return rc;
  if(!histo || !nb || !inc) return fail(JFGPU_E_INVALID, "bad histogram arguments");
  uint64_t c[CTR_COUNT];
  rc = check_deferred(t, c); if(rc) return rc;
  return scan_to_host(t, ScanArgs{SCAN_HISTO, 0ull, ~0ull, (int)(c[CTR_OVF_USED] != 0), base, ceil, inc, nb}, nb, histo);
}

int jfgpu_dump_begin(jfgpu_table* t, uint64_t lower, uint64_t upper, uint64_t* n_records, uint32_t* record_bytes) {
  int rc = use(t); if(rc) return rc;
  rc = part_flush(t); if(rc) return rc;
  uint64_t c[CTR_COUNT];
  rc = check_deferred(t, c); if(rc) return rc;
  const uint64_t nt = n_tiles_of(t);
  DevBuf<uint32_t> d_cnt;
  rc = d_cnt.alloc(nt); if(rc) return rc;
  t->dump_have_ovf = c[CTR_OVF_USED] != 0;
  if(t->slot_words > 1) HIP_TRY(hipMemsetAsync(d_cnt, 0, nt * sizeof(uint32_t), t->stream));      // (scan_kernel adds to them; tile_count_kernel writes every one)
  with_view(t, [&](const auto& T) { launch_scan(t, T, ScanArgs{SCAN_TILES, lower, upper, t->dump_have_ovf}, (unsigned long long*)nullptr, d_cnt.get()); });
  std::vector<uint32_t> h(nt);
  hipError_t e = hipMemcpyAsync(h.data(), d_cnt, nt * sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream);
  if(e == hipSuccess) e = hipStreamSynchronize(t->stream);
  if(e != hipSuccess) return fail(JFGPU_E_HIP, hipGetErrorString(e));
  t->dump_prefix.assign(nt + 1, 0);
  for(uint64_t i = 0; i < nt; ++i) t->dump_prefix[i + 1] = t->dump_prefix[i] + h[i];
  t->dump_lower = lower; t->dump_upper = upper; t->dump_tile_cursor = 0; t->dump_open = true;
  if(n_records) *n_records = t->dump_prefix[nt];
  if(record_bytes) *record_bytes = (t->g.key_bits + 7) / 8 + t->out_counter_len;
  return JFGPU_OK;
}

}  // extern "C"

namespace {

// The next chunk of the sorted dump -- as many whole tiles as hold at most capacity_records records -- into t->d_dump,
// enqueued on the table's stream (jfgpu_dump_next copies it to the host, jfgpu_dump_next_text formats it first).
// *n_read = 0 at the end.
int dump_next_chunk(jfgpu_table* t, uint64_t capacity_records, uint64_t* n_read) {
  if(!t->dump_open) return fail(JFGPU_E_INVALID, "jfgpu_dump_begin not called");
  *n_read = 0;
  const uint64_t nt = n_tiles_of(t);
  const uint64_t tsz = 1ull << t->g.tile_bits;
  if(capacity_records < tsz) return fail(JFGPU_E_INVALID, "dump buffer must hold at least one tile (" + std::to_string(tsz) + " records)");
  uint64_t t0 = t->dump_tile_cursor;
  while(t0 < nt && t->dump_prefix[t0 + 1] == t->dump_prefix[t0]) ++t0;  // skip empty tiles
  if(t0 >= nt) { t->dump_tile_cursor = nt; return JFGPU_OK; }
  // largest t1 with prefix[t1] - prefix[t0] <= capacity
  const uint64_t limit = t->dump_prefix[t0] + capacity_records;
  uint64_t t1 = std::upper_bound(t->dump_prefix.begin() + t0, t->dump_prefix.end(), limit) - t->dump_prefix.begin() - 1;
  t1 = std::min(t1, nt);
  const uint64_t ntile = t1 - t0, nrec = t->dump_prefix[t1] - t->dump_prefix[t0];
  const uint32_t key_bytes = (t->g.key_bits + 7) / 8, rec = key_bytes + t->out_counter_len;
  if(t->dump_cap_records < nrec) {
    t->dump_cap_records = 0;
    const int rc = t->d_dump.alloc(std::max<uint64_t>(nrec, capacity_records) * rec + 64); if(rc) return rc;   // (the text kernels read to the next 16-byte boundary)
    t->dump_cap_records = std::max<uint64_t>(nrec, capacity_records);
  }
  if(t->d_tile_off.cap() < ntile) { const int rc = t->d_tile_off.alloc(ntile); if(rc) return rc; }
  std::vector<uint64_t> offs(ntile);
  for(uint64_t i = 0; i < ntile; ++i) offs[i] = t->dump_prefix[t0 + i] - t->dump_prefix[t0];
  HIP_TRY(hipMemcpyAsync(t->d_tile_off, offs.data(), ntile * sizeof(uint64_t), hipMemcpyHostToDevice, t->stream));
  int rc = JFGPU_OK;
  with_view(t, [&](const auto& T) { rc = launch_dump(t, T, t0, ntile, key_bytes); });
  if(rc) return rc;
  HIP_TRY(hipGetLastError());
  t->dump_tile_cursor = t1;
  *n_read = nrec;
  return JFGPU_OK;
}

}  // namespace

extern "C" {

int jfgpu_dump_next(jfgpu_table* t, void* out, uint64_t capacity_records, uint64_t* n_read) {
  int rc = use(t); if(rc) return rc;
  if(!out || !n_read) return fail(JFGPU_E_INVALID, "null argument");
  if(!t->dump_open) return fail(JFGPU_E_INVALID, "jfgpu_dump_begin not called");
  const uint64_t cursor = t->dump_tile_cursor;
  rc = dump_next_chunk(t, capacity_records, n_read); if(rc) return rc;
  const uint32_t rec = (t->g.key_bits + 7) / 8 + t->out_counter_len;
  hipError_t e = *n_read ? hipMemcpyAsync(out, t->d_dump, *n_read * rec, hipMemcpyDeviceToHost, t->stream) : hipSuccess;
  if(e == hipSuccess) e = hipStreamSynchronize(t->stream);
  if(e != hipSuccess) { t->dump_tile_cursor = cursor; *n_read = 0; return fail(JFGPU_E_HIP, hipGetErrorString(e)); }   // (the chunk was not delivered)
  return JFGPU_OK;
}

int jfgpu_dump_end(jfgpu_table* t) {
  int rc = use(t); if(rc) return rc;
  t->dump_open = false;
  t->dump_prefix.clear(); t->dump_prefix.shrink_to_fit();
  (void)t->d_dump.reset(); t->dump_cap_records = 0;
  (void)t->d_tile_off.reset();
  return JFGPU_OK;
}

int jfgpu_set_growth(jfgpu_table* t, int on) {
  int rc = use(t); if(rc) return rc;
  t->grow_on = on != 0;
  return JFGPU_OK;
}

int jfgpu_reserve(jfgpu_table* t, uint64_t input_bytes) {
  int rc = use(t); if(rc) return rc;
  if(!t->part_ok || t->mode == MODE_DIRECT) return JFGPU_OK;
  if(t->nword && t->mode != MODE_PARTITIONED) return JFGPU_OK;      // (auto: the arena grows with the first batch that takes the path)
  rc = part_flush(t); if(rc) return rc;
  t->reserved_input = input_bytes;
  const uint32_t nb1 = 1u << t->pg.b1, nb2 = 1u << t->pg.b2;
  // pending items (upper bound: one per input byte) + the P2 output of the same size + offsets
  // (single-pass P1 batches are regions with head-room: slack + one stranded reservation per block and bucket)
  const size_t pend = align_up(input_bytes * item_size(t), 256);
  const size_t strand = (size_t)nb1 * (2 * (size_t)t->n_cu) * kGran * item_size(t);              // per batch
  const size_t headroom = t->pg.b2 ? (size_t)(pend * ((t->tun.p1_slack > 0 ? t->tun.p1_slack : 0.0) + 0.05)) + 2 * strand : 0;
  const size_t need = 2 * pend + headroom + (n_tiles_of(t) + 1 + nb1) * sizeof(uint64_t) +
                      (size_t)kMaxSeg * (align_up((2 * nb1 + 1) * sizeof(uint64_t), 256) + align_up(nb1 * 16, 256) + 1280) + ((size_t)1 << 20);
  size_t want = need;
  if(t->item128 || t->item256) {      // 16- and 32-byte items: what a whole input would need may exceed the device; the arena is then flushed more than once
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t avail = free_b + t->ws_cap > ((size_t)8 << 30) ? free_b + t->ws_cap - ((size_t)8 << 30) : 0;
    want = std::min(want, avail);
  }
  rc = ws_grow(t, want);
  if(rc < 0) return fail(JFGPU_E_ALLOC, "not enough device memory to reserve the partition workspace");
  if(rc) return rc;
  // touch every page once now: first-touch of fresh device pages costs ~40% on the first pass over them
  HIP_TRY(hipMemsetAsync(t->ws, 0, t->ws_cap, t->stream));
  if(!t->d_M1) { t->g1 = 2 * t->n_cu; rc = t->d_M1.alloc((size_t)t->g1 * kMaxBuckets); if(rc) return rc; }
  if(t->pg.b2 && !t->d_M2) { rc = t->d_M2.alloc((size_t)nb1 * 32 * nb2); if(rc) return rc; }
  return JFGPU_OK;
}

int jfgpu_table_bytes(uint32_t k, uint64_t size, uint64_t* slots, uint64_t* bytes) {
  if(k < 1 || k > 128) return fail(JFGPU_E_UNSUPPORTED, "mer length must be in [1, 128]");
  uint32_t lsize = 0;
  while(lsize < 63 && (1ull << lsize) < size) ++lsize;
  const bool nword = k > 64, wide = k > 32 && !nword;
  if(nword) { lsize = std::max(lsize, nword_min_lsize(k)); lsize = std::min<uint32_t>(lsize, 48); }
  else if(wide) { lsize = std::max(lsize, wide_min_lsize(k)); lsize = std::min<uint32_t>(lsize, 48); }
  else { lsize = std::max(lsize, geom_min_lsize(k, 0)); lsize = std::max<uint32_t>(lsize, 1); lsize = std::min<uint32_t>(lsize, 2 * k); }
  const uint64_t n = 1ull << lsize;
  uint64_t ovf = std::max<uint64_t>(kMinOvf, std::min<uint64_t>(n / 256, 1ull << 26));
  { uint64_t c = 1; while(c < ovf) c <<= 1; ovf = c; }
  if(slots) *slots = n;
  TableGeom gg;
  const bool s32 = !nword && !wide && geom_init(gg, k, lsize, 0, 0, 1, !Tuning::from_env().slot64) && gg.slot32;
  if(bytes) *bytes = n * (nword ? 32 : wide ? 16 : s32 ? 4 : 8) + ovf * 16 + (n >> std::min<uint32_t>(lsize, kMaxTileBits)) + (size_t)(2 * k + 7) / 8 * 256 * 8 * 2;
  return JFGPU_OK;
}

int jfgpu_set_spill(jfgpu_table* t, int (*fn)(void*), void* user) {
  int rc = use(t); if(rc) return rc;
  t->spill_fn = fn; t->spill_user = user;
  return JFGPU_OK;
}

int jfgpu_reference_matrix(uint32_t lsize, uint32_t key_len, uint64_t* columns) {
  if(!columns || lsize < 1 || lsize > 64 || key_len < 2 || key_len > 256) return fail(JFGPU_E_INVALID, "bad matrix dimensions");
  GlibcRandom rng;
  const Gf2Matrix m = lsize >= key_len ? gf2_identity(lsize, key_len) : gf2_reference_matrix(lsize, key_len, rng);
  for(uint32_t i = 0; i < key_len; ++i) columns[i] = m.columns[i];
  return JFGPU_OK;
}

int jfgpu_set_operation(jfgpu_table* t, int op) {
  int rc = use(t); if(rc) return rc;
  if(op < 0 || op > 2) return fail(JFGPU_E_INVALID, "operation must be 0 (count), 1 (prime) or 2 (update)");
  if(op != t->operation) { rc = part_flush(t); if(rc) return rc; }     // pending adds belong to the old operation
  t->operation = op;
  return JFGPU_OK;
}

int jfgpu_set_mode(jfgpu_table* t, int mode) {
  int rc = use(t); if(rc) return rc;
  if(mode < 0 || mode > 2) return fail(JFGPU_E_INVALID, "mode must be 0 (auto), 1 (direct) or 2 (partitioned)");
  if(mode == MODE_PARTITIONED && !t->part_ok) return fail(JFGPU_E_UNSUPPORTED, "table geometry has no partitioned path");
  rc = part_flush(t); if(rc) return rc;
  t->mode = mode;
  return JFGPU_OK;
}

int jfgpu_profile_enable(jfgpu_table* t, int on) {
  int rc = use(t); if(rc) return rc;
  t->prof_on = on != 0;
  return JFGPU_OK;
}

int jfgpu_profile_get(jfgpu_table* t, int which, double* ms, uint64_t* launches, uint64_t* units) {
  int rc = use(t); if(rc) return rc;
  if(which < 0 || which >= kNumProf) return fail(JFGPU_E_INVALID, "bad profile slot");
  HIP_TRY(hipStreamSynchronize(t->stream));
  prof_collect(t);
  if(ms) *ms = t->prof_ms[which];
  if(launches) *launches = t->prof_launches[which];
  if(units) *units = t->prof_units[which];
  return JFGPU_OK;
}

int jfgpu_get_counters(jfgpu_table* t, uint64_t* out, uint32_t n) {
  int rc = use(t); if(rc) return rc;
  if(!out) return fail(JFGPU_E_INVALID, "null argument");
  uint64_t c[CTR_COUNT];
  rc = read_counters(t, c); if(rc) return rc;
  const uint64_t v[JFGPU_N_COUNTERS] = {c[CTR_FULL], c[CTR_MERS], c[CTR_OVF_FULL], c[CTR_OVF_USED], c[CTR_MISROUTED], c[CTR_DIRECT],
                                        c[CTR_T_ITEMS], c[CTR_T_QUEUED], t->flushes_plain, t->flushes_heavy,
                                        t->n_p2_roles, t->n_p2_ring, t->n_p2_sort, t->n_p2_exact, t->n_p1_ring, t->n_p1_other, t->n_tile_dense, t->n_tile_nword};
  for(uint32_t i = 0; i < n; ++i) out[i] = i < JFGPU_N_COUNTERS ? v[i] : 0;
  return JFGPU_OK;
}

int jfgpu_profile_reset(jfgpu_table* t) {
  int rc = use(t); if(rc) return rc;
  HIP_TRY(hipStreamSynchronize(t->stream));
  prof_collect(t);
  for(int i = 0; i < kNumProf; ++i) { t->prof_ms[i] = 0; t->prof_launches[i] = 0; t->prof_units[i] = 0; }
  t->prof_log.clear();
  return JFGPU_OK;
}

int jfgpu_profile_spans(jfgpu_table* t, int* which, double* ms, size_t cap, size_t* n) {
  int rc = use(t); if(rc) return rc;
  if(!n) return fail(JFGPU_E_INVALID, "null argument");
  HIP_TRY(hipStreamSynchronize(t->stream));
  prof_collect(t);
  *n = t->prof_log.size();
  for(size_t i = 0; i < t->prof_log.size() && i < cap; ++i) { if(which) which[i] = t->prof_log[i].first; if(ms) ms[i] = t->prof_log[i].second; }
  return JFGPU_OK;
}

int jfgpu_gen_reads_dev(jfgpu_table* t, char* d_out, uint64_t first_read, uint64_t n_reads, uint32_t read_len, uint64_t seed) {
  int rc = use(t); if(rc) return rc;
  if(!n_reads) return JFGPU_OK;
  if(!d_out) return fail(JFGPU_E_INVALID, "null buffer");
  if(read_len < 1 || read_len > 2048) return fail(JFGPU_E_INVALID, "read_len must be in [1, 2048]");
  if(((uintptr_t)d_out & 15) != 0) return fail(JFGPU_E_INVALID, "gen_reads: output must be 16-byte aligned");
  const uint64_t vecs = (n_reads * ((uint64_t)read_len + 1) + 15) / 16;
  hipLaunchKernelGGL(gen_reads_kernel, dim3(grid_for(t, (vecs + kBlock - 1) / kBlock)), dim3(kBlock), 0, t->stream,
                     (uint8_t*)d_out, first_read, n_reads, read_len, seed);
  HIP_TRY(hipGetLastError());
  return JFGPU_OK;
}

int jfgpu_gen_genome_reads_dev(jfgpu_table* t, char* d_out, uint64_t first_read, uint64_t n_reads, uint32_t read_len,
                               uint64_t genome_len, double substitution_rate, uint64_t seed) {
  int rc = use(t); if(rc) return rc;
  if(!n_reads) return JFGPU_OK;
  if(!d_out) return fail(JFGPU_E_INVALID, "null buffer");
  if(read_len < 1 || read_len > 2048 || genome_len < read_len) return fail(JFGPU_E_INVALID, "read_len must be in [1, 2048] and <= genome_len");
  if(substitution_rate < 0 || substitution_rate > 0.5) return fail(JFGPU_E_INVALID, "substitution rate must be in [0, 0.5]");
  if(((uintptr_t)d_out & 15) != 0) return fail(JFGPU_E_INVALID, "gen_genome_reads: output must be 16-byte aligned");
  const uint64_t vecs = (n_reads * ((uint64_t)read_len + 1) + 15) / 16;
  hipLaunchKernelGGL(gen_genome_reads_kernel, dim3(grid_for(t, (vecs + kBlock - 1) / kBlock)), dim3(kBlock), 0, t->stream,
                     (uint8_t*)d_out, first_read, n_reads, read_len, genome_len, (uint32_t)lrint(substitution_rate * 65536.0), seed);
  HIP_TRY(hipGetLastError());
  return JFGPU_OK;
}

int jfgpu_gups(jfgpu_table* t, uint64_t n_updates, int mode, double* ups) {
  int rc = use(t); if(rc) return rc;
  if(!ups) return fail(JFGPU_E_INVALID, "null out");
  DevBuf<unsigned long long> d_sink;
  rc = d_sink.alloc(1); if(rc) return rc;
  HIP_TRY(hipMemsetAsync(d_sink, 0, sizeof(unsigned long long), t->stream));
  Event a, b;
  if((rc = a.create()) || (rc = b.create())) return rc;
  const uint64_t mask = (((1ull << t->g.lsize_l) * slot_bytes_of(t)) >> 3) - 1;    // 64-bit words of the table's allocation
  t->pristine = false;
  HIP_TRY(hipMemsetAsync(t->dt.dirty, 1, (size_t)1 << (t->g.lsize_l - t->g.tile_bits), t->stream));
  const int grid = grid_for(t, (n_updates + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(gups_kernel, dim3(grid), dim3(kBlock), 0, t->stream, t->dt.slots, mask, std::min<uint64_t>(n_updates, 1u << 20), mode, 1ull, d_sink.get());  // warm-up
  HIP_TRY(hipEventRecord(a, t->stream));
  hipLaunchKernelGGL(gups_kernel, dim3(grid), dim3(kBlock), 0, t->stream, t->dt.slots, mask, n_updates, mode, 42ull, d_sink.get());
  HIP_TRY(hipEventRecord(b, t->stream));
  HIP_TRY(hipEventSynchronize(b));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, a, b));
  *ups = ms > 0 ? (double)n_updates / (ms * 1e-3) : 0;
  return JFGPU_OK;
}

int jfgpu_malloc_host(size_t bytes, void** out) {       // pinned: device copies to / from it run at PCIe speed
  if(!out) return fail(JFGPU_E_INVALID, "null out");
  *out = nullptr;
  HIP_TRY(hipHostMalloc(out, bytes ? bytes : 16, hipHostMallocDefault));
  return JFGPU_OK;
}
int jfgpu_free_host(void* p) {
  if(p) HIP_TRY(hipHostFree(p));
  return JFGPU_OK;
}
int jfgpu_malloc_dev(jfgpu_table* t, size_t bytes, void** out) {
  int rc = use(t); if(rc) return rc;
  if(!out) return fail(JFGPU_E_INVALID, "null out");
  HIP_TRY(hipMalloc(out, bytes ? bytes : 16));
  return JFGPU_OK;
}
int jfgpu_free_dev(jfgpu_table* t, void* p) {
  int rc = use(t); if(rc) return rc;
  HIP_TRY(hipStreamSynchronize(t->stream));
  HIP_TRY(hipFree(p));
  return JFGPU_OK;
}
int jfgpu_memcpy_h2d(jfgpu_table* t, void* d_dst, const void* src, size_t bytes) {
  int rc = use(t); if(rc) return rc;
  HIP_TRY(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  return JFGPU_OK;
}
int jfgpu_memcpy_d2h(jfgpu_table* t, void* dst, const void* d_src, size_t bytes) {
  int rc = use(t); if(rc) return rc;
  HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  return JFGPU_OK;
}

}  // extern "C"

#include "abi_bloom.inl"
#include "abi_parser.inl"
#include "abi_sam.inl"
#include "abi_comm.inl"
#include "abi_merge.inl"
#include "abi_text.inl"
#include "abi_qtext.inl"
#include "abi_sorted.inl"
