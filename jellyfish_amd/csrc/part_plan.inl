// jellyfish_amd/csrc/part_plan.inl -- what the partitioned insert path decides, apart from doing it.  Included by jfgpu.hip
// inside its anonymous namespace, after the kernel headers (whose constants size the plans) and before host_partition.inl,
// which gathers the facts, asks for a plan and carries it out.  The plan functions see a PartFacts and plain numbers: no
// table, no stream, no device memory, no allocation -- tests/host/plan_check.cc calls them on facts written out by hand.
size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The arena's bump allocation on numbers (ws_alloc is this on a table): where a block of `bytes` starts, kNoBlock when
// there is no room for it (`used` then stays).
constexpr size_t kNoBlock = ~(size_t)0;
size_t arena_take(size_t& used, size_t cap, size_t bytes) {
  const size_t at = align_up(used, 256);
  if(at + bytes > cap) return kNoBlock;
  used = at + bytes;
  return at;
}

struct PartFacts {
  PartGeom pg{};
  uint32_t item_bytes = 4;       // 4 / 8 / 16 / 32
  bool slot32 = false;
  int mode = 0, n_cu = 0, g1 = 0;
  uint64_t n_tiles = 0;
  bool returning = false, wide = false, filter = false;
  bool nword = false;            // the key class: keys of three and four words (32-byte items); wide: two words (16-byte items); else one
  int filter_kind = 0;           // (a filter of kind 1 changes as it is asked: count --bf-size)
  uint32_t nbytes = 0;
  bool hash_xs = false, canonical = false;
  uint32_t lsize_g = 0, lsize_l = 0, tile_bits = 0;
  uint32_t tag_bits = 0;         // where an item's P2 sub-bucket starts (keys of two and more words: tag_full)
  double items_per_byte = 0;
  size_t ws_cap = 0, ws_used = 0;
  uint64_t reserved_input = 0;
  Tuning tun;
};

// ---- which instantiation: a kernel's template arguments as a value ---------------------------------------------------
// The plan names an instantiation by its integer arguments (bools as 0 / 1); the executor lists the instantiations that
// exist as Inst<...> types and pick() calls f with the one the plan named.  None: false, which the caller reports -- a
// kernel that is not there is an error, never another kernel.
typedef std::array<int, 5> TArgs;      // (unused trailing entries are 0)
template <int... V> struct Inst {
  static constexpr int v[sizeof...(V)] = {V...};
  static bool is(const TArgs& a) { for(size_t i = 0; i < sizeof...(V); ++i) if(a[i] != v[i]) return false; return true; }
};
template <class... Is, class F> bool pick(const TArgs& want, F&& f) { return ((Is::is(want) && (f(Is{}), true)) || ...); }
// run-time flags as template arguments: f(std::bool_constant<a>{}, ...)
template <class F> void with_flags(bool a, F&& f) { if(a) f(std::true_type{}); else f(std::false_type{}); }
template <class F> void with_flags(bool a, bool b, F&& f) { with_flags(a, [&](auto A) { with_flags(b, [&](auto B) { f(A, B); }); }); }

// ---- P1: one batch ---------------------------------------------------------------------------------------------------
enum FlushWhy { kFlushNo = 0, kFlushSegments, kFlushWideShare, kFlushEven, kFlushArenaFull };
enum P1Kind { kP1Ring, kP1KeysGranule, kP1Granule64, kP1WideGranule, kP1ExactSorted, kP1ExactKeysSorted, kP1ExactPlain, kP1NWordGranule };
struct PendingSum { size_t n = 0; uint64_t input_bytes = 0; };     // the pending batches: how many, made from how many sequence bytes
struct P1Plan {
  int flush = kFlushNo;          // apply what is pending first, and why (kFlushSegments: then ask again)
  bool refuse = false;           // the batch goes to the direct kernel (part_ingest returns -1)
  uint32_t gran_cap = 0;         // single-pass P1: items per bucket region; 0: the exact two-pass scheme
  size_t bytes = 0, arena = 0;   // of the batch's items; of all its arena blocks (the arena grows to this when smaller)
  int kind = kP1ExactPlain;
  TArgs targs{};                 // kP1Ring <BLOOM, N, CN>, kP1KeysGranule <RT, N>, kP1Granule64 <RT, BL, N>, kP1WideGranule <RT, BL, XS>, kP1NWordGranule <RT>,
                                 // kP1ExactSorted <RT, BL, N>, kP1ExactKeysSorted <N>, kP1ExactPlain p1_kernel's <SC = 1, FK, RT, BL, N>
  TArgs count_targs{};           // the exact kinds' first pass: p1_kernel's <SC = 0, FK, RT, BL, N>
  size_t lds = 0;
  uint32_t grid = 0;
};

// Single-pass P1 (p1_ring_kernel, p1_keys_granule_kernel, ...): items per bucket region, 0 when the batch takes the exact
// two-pass scheme.  Every block may strand part of one reservation per bucket, so small batches would be
// mostly holes: auto mode wants the mean bucket load to be at least 4x that.
uint32_t granule_cap(const PartFacts& f, bool from_keys, uint64_t max_items) {
  const bool wide = f.item_bytes >= 16;                                   // (keys of two words, and of three and four)
  if(wide) { if(f.pg.b1 > 10 || !f.g1) return 0; }                      // the only P1 these keys have
  else if(f.pg.b2 == 0 || f.pg.b1 > 10 || f.tun.p1_single == 0 || !f.g1) return 0;
  else if(f.item_bytes == 8 && from_keys) return 0;                       // 64-bit items: single-pass from sequence only
  const uint64_t nb = 1ull << f.pg.b1, strand = (uint64_t)f.g1 * kGran;
  // Sequence input: one item per byte is the upper bound, what earlier flushes saw per byte (+10 %) the estimate -- reads
  // of length L give (L - k + 1) / (L + 1) items per byte, 0.58 at k = 63.  An underestimate is safe: what does not fit
  // a region is inserted directly (granule_emit), it only costs speed.
  if(!from_keys && f.items_per_byte > 0) max_items = std::min<uint64_t>(max_items, (uint64_t)((double)max_items * (f.items_per_byte * 1.10 + 0.005)) + 4096);
  const uint64_t mean = (max_items + nb - 1) / nb;
  // a filtered pass (count --bc) stores few items, but the exact two-pass scheme would ask the filter twice per k-mer
  // (random reads: what the pass costs); stranded reservations are at most g1 * nb * kGran items per batch
  const bool filtered = !from_keys && f.filter;
  if(f.tun.p1_single < 0 && mean < 4 * strand && !filtered && !(wide && f.mode == MODE_PARTITIONED)) return 0;
  const double want = (double)mean * (1.0 + f.tun.p1_slack) + (double)strand;
  uint64_t cap = want < (double)kGran ? kGran : (uint64_t)want;
  cap = (cap + kGran - 1) / kGran * kGran;
  if(cap > 0xFFFF0000ull) return 0;
  return (uint32_t)cap;
}

// the common key widths get kernels with the byte count of the hash compiled in (no per-k-mer switch)
int compiled_nbytes(uint32_t nbytes, uint32_t from) { return nbytes >= from && nbytes <= 8 ? (int)nbytes : 0; }

P1Plan p1_plan(const PartFacts& f, bool from_keys, uint64_t max_items, int64_t lo, int64_t hi, PendingSum pend) {
  P1Plan p;
  if(pend.n >= (size_t)kMaxSeg) { p.flush = kFlushSegments; return p; }
  const bool wide = f.item_bytes >= 16, item32 = f.item_bytes == 4;
  const uint32_t nb = 1u << f.pg.b1, gcap = p.gran_cap = granule_cap(f, from_keys, max_items);
  if(wide && (!gcap || from_keys)) { p.refuse = true; return p; }       // keys of two and more words: single-pass P1 from sequence or the direct kernel
  if(f.nword && f.filter) { p.refuse = true; return p; }                // ... and of three and four words: no filtered P1
  // a one-pass Bloom filter (count --bf-size) changes as it is asked: the two-pass P1 would ask it twice per k-mer
  if(!gcap && !from_keys && f.filter && f.filter_kind == 1) { p.refuse = true; return p; }
  p.bytes = gcap ? (size_t)nb * gcap * f.item_bytes : max_items * f.item_bytes;
  const size_t need = p.arena = align_up(p.bytes, 256) + align_up((2 * nb + 1) * sizeof(uint64_t), 256) + (gcap ? align_up(nb * 16, 256) : 0) + 1024;
  // 16-byte items: the arena is what limits the k-mers per flush, and every flush streams the whole table.  It may be
  // smaller than what the whole input needs, so part of it is kept for the flush's P2 output (an eighth is enough: P2 and
  // the tile insert then go group by group, flush_plan)
  const size_t ws_limit = wide && f.pg.b2 ? f.ws_cap - f.ws_cap / 8 : f.ws_cap;
  if(wide && pend.n && f.ws_used + need > ws_limit) p.flush = kFlushWideShare;
  // ... so when the announced input (jfgpu_reserve) needs n flushes, make them n equal ones: 6 + 3 + 1 batches cost a
  // third more table traffic than 5 + 5
  else if(wide && !from_keys && f.reserved_input && pend.n && need > 0) {
    const double per_flush = (double)ws_limit / (double)need * (double)(hi - lo);       // input bytes one flush can hold
    if(per_flush > 0 && (double)f.reserved_input > per_flush) {
      const double n = std::ceil((double)f.reserved_input / per_flush);
      if((double)pend.input_bytes + (double)(hi - lo) > (double)f.reserved_input / n * 1.02) p.flush = kFlushEven;
    }
  }
  if(!p.flush && pend.n && f.ws_used + need > f.ws_cap) p.flush = kFlushArenaFull;      // apply what is pending, arena is empty again
  const int rt = f.returning, bl = f.filter && !from_keys;     // the filter applies to the sequence feed only
  p.grid = (uint32_t)f.g1;
  if(gcap && f.nword) {
    p.kind = kP1NWordGranule; p.targs = {rt}; p.lds = p1_nword_lds(f.nbytes);
  } else if(gcap && wide) {
    const int xs = f.hash_xs && !bl;
    p.kind = kP1WideGranule; p.targs = {rt, bl, xs}; p.lds = (size_t)kWideChunk * 18 + (size_t)f.nbytes * 2048;
  } else if(gcap && !item32) {
    p.kind = kP1Granule64; p.lds = (size_t)kG64Chunk * 10;
    p.targs = bl ? TArgs{rt, 1, 0} : f.hash_xs ? TArgs{rt, 0, kHashXS} : rt ? TArgs{1, 0, 0} : TArgs{0, 0, compiled_nbytes(f.nbytes, 7)};
  } else if(gcap && from_keys) {
    p.kind = kP1KeysGranule; p.lds = (size_t)kPTilePos * 6;
    p.targs = rt ? TArgs{1, 0} : TArgs{0, compiled_nbytes(f.nbytes, 6)};
  } else if(gcap) {
    // (32-bit items exist for keys of at most 42 bits: six key bytes is the only width worth a compiled-in hash)
    // the xor-shift matrix is evaluated in registers (kmer_core.hpp: xs_hash); on the key's two dwords when the position has
    // more than 32 bits, which is the metric's geometry
    const bool xs = f.hash_xs && !bl, xs_hi = xs && f.lsize_g > 32 && f.lsize_g < 64 && f.lsize_l - f.pg.b1 < 32;
    p.kind = kP1Ring; p.grid = (uint32_t)f.n_cu; p.lds = (size_t)nb * 128 + 128;
    p.targs = xs_hi ? TArgs{0, kHashXS, f.canonical} : xs ? TArgs{0, kHashXSLow, 2} : f.nbytes == 6 && !bl ? TArgs{0, 6, f.canonical} : TArgs{bl, 0, 2};
  } else {
    const int n68 = f.nbytes == 6 ? 6 : f.nbytes == 7 ? 7 : 8;
    p.count_targs = !bl && f.nbytes >= 6 ? TArgs{0, from_keys, 0, 0, n68} : TArgs{0, from_keys, 0, bl, 0};
    if(item32 && !from_keys) {          // write-combining scatter (whole runs per bucket)
      p.kind = kP1ExactSorted; p.lds = (size_t)kPTilePos * 6;
      p.targs = !rt && !bl && f.nbytes >= 6 ? TArgs{0, 0, n68} : TArgs{rt, bl, 0};
    } else if(item32) {                 // encoded keys, 32-bit items: same write-combining scatter
      p.kind = kP1ExactKeysSorted; p.lds = (size_t)kPTilePos * 6; p.targs = {compiled_nbytes(f.nbytes, 6)};
    } else { p.kind = kP1ExactPlain; p.targs = {1, from_keys, rt, bl, 0}; }
  }
  return p;
}

// ---- the flush -------------------------------------------------------------------------------------------------------
// Single-pass P2 of 4-byte items through per-destination rings (kernels_p1ring.hip.hpp): one workgroup per bucket with
// loader and storer waves when that fills the chip (p2_ring_roles_kernel), else several workgroups per bucket sharing the
// regions through reservations (p2_ring_kernel).  Rings hold 32 items: the kernels are for buckets of 1024 destinations
// (512 with the loader / storer kernel's short rounds) -- p2_rings_fit says so, else the sort.
constexpr uint32_t kG2Blocks = 4;      // workgroups per bucket of the single-pass P2 kernels that share regions
constexpr uint32_t kG2Single = 4;      // ... of the sort-based one
constexpr uint32_t kG2Exact = 32;      // ... of the exact count + scatter (rows of M2 per bucket)
bool p2_rings_roles(const PartFacts& f, uint32_t b2e, uint32_t nbk) { return f.tun.p2_ring != 3 && nbk >= 2 * (uint32_t)f.n_cu && (b2e == 10 || b2e == 9); }
bool p2_rings_fit(const PartFacts& f, uint32_t b2e, uint32_t nbk) { return f.tun.p2_ring && (b2e == 10 || p2_rings_roles(f, b2e, nbk)); }

enum Route { kRouteNothing, kRouteDirect, kRouteSingleLevel, kRouteTwoLevel };
enum P2Kind { kP2Roles, kP2SharedRing, kP2Sort, kP2Exact };
struct FlushAllow { bool single_one_off = true, exact_one_off = true; };      // options still open: struck when their allocation failed
struct FlushPlan {
  int route = kRouteNothing;
  // kRouteTwoLevel:
  bool pair = false;             // P2 routes to pairs of adjacent tiles, the tile kernel owns a pair
  uint32_t cap2 = 0;             // single-pass P2: items per destination region; 0: the exact count + scatter
  uint64_t n_dest = 0;
  uint32_t b2e = 0;              // pg2.b2: P2's bits (one fewer with pairs)
  uint32_t p2_tag_bits = 0;      // where an item's P2 sub-bucket starts
  uint32_t n_groups = 1;         // the P1 buckets go through P2 and the tile insert in this many groups ...
  bool share = false;            // ... which share one output buffer (group g's tiles are in before group g + 1 is partitioned)
  bool two_streams = false;      // ... or run P2 on the table's stream and the tile insert on a second one
  bool one_off = false;          // the blocks below do not fit the arena: allocated for this flush alone
  bool no_memory = false;        // ... and that was struck: the flush fails
  // the blocks, in the order taken: gcur2 (u32) / off2 (u64) / out2 (items) with cap2, else goff (u64) / base (u64) / tmp (items)
  size_t block_bytes[3] = {0, 0, 0}, block_at[3] = {kNoBlock, kNoBlock, kNoBlock};
  uint64_t tmp_items = 0;        // exact P2: items of the largest group (of the flush when the groups do not share)
};
struct GroupPlan {
  uint32_t b0 = 0, nbk = 0;      // the group's P1 buckets
  uint64_t items = 0;
  int p2 = kP2Exact;
  TArgs p2_targs{};              // kP2Roles <NV, PD>; kP2Exact <per_thread> of the scatter
  uint32_t grid_x = 0, grid_y = 0;
  size_t lds = 0;
  uint64_t d0 = 0, nd = 0;       // the group's destinations
  uint64_t tile0 = 0;            // the tile insert: first tile, units (tiles or pairs of them) ...
  uint32_t ntile = 0, sample = 0;     // ... and how many of them go first with the sample counters on (0: no sampling)
  bool dense = false;            // P2 leaves regions without holes (SegList::dense) ...
  bool tile_dense = false;       // ... and the plain tile kernel's hole-free instantiation takes them
};

uint32_t tile_sample_units(const PartFacts& f, uint32_t ntile, uint32_t n_seg) { return f.tun.tile_adapt == 1 && ntile >= 8192 && n_seg == 1 ? ntile / 64 : 0; }

FlushPlan flush_plan(const PartFacts& f, uint64_t total, const uint64_t* bucket_tot, size_t nbatch, bool all_granule, FlushAllow allow) {
  FlushPlan p;
  (void)nbatch; (void)all_granule;       // (what a group's P2 is depends on them: group_plan)
  const uint32_t nb1 = 1u << f.pg.b1, item = f.item_bytes;
  if(total == 0) return p;
  // too few items to be worth streaming the tiles: global atomics straight from the items
  if(f.mode != MODE_PARTITIONED && total < f.n_tiles * 256) { p.route = kRouteDirect; return p; }
  // single-level table (at most 2^11 tiles): the P1 buckets are the tiles
  if(f.pg.b2 == 0) { p.route = kRouteSingleLevel; return p; }
  // breadth-first: every P1 bucket through P2 in one launch per pass, then every tile in one launch
  p.route = kRouteTwoLevel;
  // 32-bit items into 32-bit slots: P2 routes to pairs of adjacent tiles (half as many destinations, and chunks of 28 Ki
  // items), so the runs it writes are ~112 bytes on average instead of 32; the tile kernel owns a pair (64 KiB) in LDS
  p.pair = item == 4 && f.slot32 && f.pg.b2 >= 1 && f.tun.tile_pair;
  p.b2e = f.pg.b2 - (p.pair ? 1 : 0);
  p.p2_tag_bits = f.tag_bits + (p.pair ? 1 : 0);
  p.n_dest = p.pair ? f.n_tiles >> 1 : f.n_tiles;
  const uint32_t forced = f.tun.flush_share;      // (tests)
  // Single-pass P2 (32-bit items into pairs of tiles; 8- and 16-byte items into tiles): fixed regions of cap2 items per
  // destination, reservations of kGran items (p2_granule_kernel).  Worth it when the regions are mostly items: every
  // block may strand one reservation per destination.  When the regions of the whole table do not fit the arena beside
  // what is pending, the P1 buckets go through P2 and the tile insert in groups sharing one buffer.
  // (The single-pass kernel places one destination per thread (GranuleLds: kGranMaxB = 1024); from 2^34 slots on b2 is 11,
  // and what is not routed to pairs takes the exact scheme, whose kernels go to kMaxBuckets = 2048 destinations)
  // (32-byte items have the exact scheme only)
  const bool single_ok = f.tun.p2_single && ((item >= 8 && item <= 16) || p.pair) && f.tun.flush_groups <= 1 && (1u << p.b2e) <= (uint32_t)kGranMaxB;
  uint32_t single_groups = 1;
  if(single_ok) {
    // what a destination's region may lose to reservations nobody fills: one granule per block -- two with the ring kernel,
    // whose owners ask for the next reservation a round ahead -- and the holes behind the blocks' last units
    const bool ring = item == 4 && f.tun.p2_ring;
    const uint64_t mean = total / p.n_dest, strand = (uint64_t)kG2Single * kGran * (ring ? 2 : 1) + (ring ? kGran : 0);
    // ... except with the loader / storer kernel: one workgroup owns a bucket's regions, nothing is reserved, a region
    // ends behind its last item and loses nothing -- worth it from a few units per destination (a 155 Mbp sample in the
    // metric's 2^34-slot table takes the timed job's kernels: bench.py's digest check against the reference)
    const bool roles_geom = item == 4 && p.pair && p2_rings_fit(f, p.b2e, nb1) && p2_rings_roles(f, p.b2e, nb1);
    if(mean >= (roles_geom ? 32 : 8 * strand) || f.tun.p2_single > 1) {
      // head-room over the mean load: a pair of tiles takes ~8 K items a flush, 1 % standard deviation on uniform reads --
      // but on high-coverage input its ~100 hot k-mers come 80 times each (10 %), and what overflows a region is
      // inserted with global atomics: with 8 % head-room P2 took 38 ms on distribution G instead of 29
      const double slack = f.tun.p2_slack >= 0 ? f.tun.p2_slack : (item <= 8 ? 0.30 : 0.08);
      p.cap2 = (uint32_t)(((uint64_t)((double)mean * (1.0 + slack)) + strand + 2 * kGran - 1) / kGran * kGran);
      if(f.tun.p2_cap) p.cap2 = f.tun.p2_cap;
      size_t used = f.ws_used;
      p.block_bytes[0] = 2 * p.n_dest * sizeof(unsigned int); p.block_bytes[1] = 2 * p.n_dest * sizeof(uint64_t);
      p.block_at[0] = arena_take(used, f.ws_cap, p.block_bytes[0]);
      p.block_at[1] = arena_take(used, f.ws_cap, p.block_bytes[1]);
      const size_t end = align_up(used, 256) + 4096;
      const size_t free_b = f.ws_cap > end ? f.ws_cap - end : 0;
      uint32_t G = forced && forced <= nb1 / 8 ? forced : 1;
      while(!forced && G <= nb1 / 8 && (p.n_dest / G) * p.cap2 * item > free_b) G *= 2;
      p.block_bytes[2] = (p.n_dest / G) * p.cap2 * item;
      if(p.block_at[0] != kNoBlock && p.block_at[1] != kNoBlock && G <= std::max<uint32_t>(1, nb1 / 8)) p.block_at[2] = arena_take(used, f.ws_cap, p.block_bytes[2]);
      if(p.block_at[2] != kNoBlock) single_groups = G;
      else {                                   // no room for the regions in the arena: exact P2 (forced: one-off allocations)
        single_groups = forced && forced <= nb1 / 8 ? forced : 1;
        p.block_bytes[2] = (p.n_dest / single_groups) * p.cap2 * item;
        if(f.tun.p2_single > 1 && allow.single_one_off) p.one_off = true;
        else { p.cap2 = 0; single_groups = 1; }
      }
    }
  }
  // Exact P2.  When the arena cannot hold a P2 output of the whole flush beside what is pending, the P1 buckets go through
  // P2 and the tile insert in groups that share one small output buffer: 16-byte items at 10 Gbp then need 104 GB (P1
  // regions) + 12 GB instead of 104 + 94, the whole job fits one flush, and the table is streamed once instead of twice.
  uint32_t share_groups = p.cap2 && single_groups > 1 ? single_groups : 0;      // (single-pass groups: the shared buffer holds regions)
  if(!p.cap2) {
    p.tmp_items = std::max<uint64_t>(total, 1);
    const size_t fixed = align_up((f.n_tiles + 1) * sizeof(uint64_t), 256) + align_up(nb1 * sizeof(uint64_t), 256) + 1024;
    size_t used = align_up(f.ws_used, 256);
    const size_t free_b = f.ws_cap > used + fixed ? f.ws_cap - used - fixed : 0;
    if(((size_t)total * item > free_b || forced) && f.tun.flush_groups <= 1) {
      for(uint32_t G = 2; G <= nb1 / 8; G *= 2) {
        uint64_t mx = 0;
        for(uint32_t g = 0; g < G; ++g) { uint64_t sum = 0; for(uint32_t j = g * (nb1 / G); j < (g + 1) * (nb1 / G); ++j) sum += bucket_tot[j]; mx = std::max(mx, sum); }
        if(forced ? G == forced : mx * item <= free_b) { share_groups = G; p.tmp_items = std::max<uint64_t>(mx, 1); break; }
      }
    }
    used = f.ws_used;
    p.block_bytes[0] = (f.n_tiles + 1) * sizeof(uint64_t); p.block_bytes[1] = nb1 * sizeof(uint64_t); p.block_bytes[2] = p.tmp_items * item;
    for(int i = 0; i < 3; ++i) p.block_at[i] = arena_take(used, f.ws_cap, p.block_bytes[i]);
    if(p.block_at[0] == kNoBlock || p.block_at[1] == kNoBlock || p.block_at[2] == kNoBlock) {     // arena too small for the flush temporaries: one-off allocation
      if(!forced) { share_groups = 0; p.tmp_items = std::max<uint64_t>(total, 1); p.block_bytes[2] = p.tmp_items * item; }
      p.one_off = true; p.no_memory = !allow.exact_one_off;
    }
  }
  // Optionally (JFGPU_FLUSH_GROUPS > 1) the P1 buckets go through P2 and the tile insert in groups, P2 on the
  // table's stream and the tile insert on a second one, so that group g's tiles are inserted while group g+1
  // is partitioned (one P2-scatter block, 88 KB LDS, and one tile block, 64 KB, fit a CU together).
  p.share = share_groups != 0;
  p.n_groups = share_groups ? share_groups : f.tun.flush_groups > 1 && nb1 >= (uint32_t)f.tun.flush_groups * 8 ? (uint32_t)f.tun.flush_groups : 1;
  p.two_streams = p.n_groups > 1 && !p.share;
  return p;
}

// Group g of a two-level flush: its P2 and its tile insert.
// The ring kernels of P2 read every all-ones item as a hole and load 16 bytes at a time: right for granule batches (fixed
// regions, holes marked so), wrong for an exact two-pass batch, which stores every item -- the all-ones one too when
// items are 32 bits wide -- at arbitrary offsets.  The loader / storer kernel takes such a segment item by item
// (load_exact); a flush holding one keeps the sort-based kernel where the shared-ring kernel would run.
GroupPlan group_plan(const PartFacts& f, const FlushPlan& p, uint32_t g, const uint64_t* bucket_tot, bool all_granule) {
  GroupPlan q;
  const uint32_t nb1 = 1u << f.pg.b1, gsz = nb1 / p.n_groups, item = f.item_bytes;
  q.b0 = g * gsz; q.nbk = g + 1 == p.n_groups ? nb1 - q.b0 : gsz;
  for(uint32_t j = q.b0; j < q.b0 + q.nbk; ++j) q.items += bucket_tot[j];
  q.d0 = (uint64_t)q.b0 << p.b2e; q.nd = (uint64_t)q.nbk << p.b2e;
  q.grid_y = q.nbk;
  if(!p.cap2) {
    // 8- and 16-byte items: chunks of 112 KiB (longer runs per destination); 32-byte items: 96 KiB
    const int per_thread = p.pair ? kP2PairPer : item == 4 ? 16 : item == 8 ? 14 : item == 16 ? 7 : kP2NWordPer;
    q.p2 = kP2Exact; q.p2_targs = {per_thread}; q.grid_x = kG2Exact; q.lds = (size_t)kPBlock * per_thread * item;
  } else if(item == 4 && p2_rings_fit(f, p.b2e, q.nbk) && (all_granule || p2_rings_roles(f, p.b2e, q.nbk))) {
    const bool roles = p2_rings_roles(f, p.b2e, q.nbk);
    q.p2 = roles ? kP2Roles : kP2SharedRing; q.p2_targs = {p.b2e == 10 ? 2 : 1, f.tun.p2_depth};
    if(roles) { q.grid_x = q.nbk; q.grid_y = 1; } else q.grid_x = kG2Blocks;
    q.lds = ((size_t)1 << p.b2e) * 128 + 128;
    q.dense = roles;
  } else {
    q.p2 = kP2Sort; q.grid_x = kG2Single; q.lds = (size_t)kPBlock * (item == 4 ? kP2PairPer : item == 8 ? kP2MidPer : kP2WidePer) * item;
  }
  q.tile0 = (uint64_t)q.b0 << f.pg.b2;
  q.ntile = (uint32_t)q.nd;                               // units of the tile kernel: tiles, or pairs of tiles
  q.sample = f.wide || f.nword ? 0 : tile_sample_units(f, q.ntile, 1);
  q.tile_dense = q.dense && item == 4 && p.pair && f.tun.tile_adapt != 2;
  return q;
}
