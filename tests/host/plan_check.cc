// tests/host/plan_check.cc -- TEST-ONLY: the plans of the partitioned insert path (jellyfish_amd/csrc/part_plan.inl) on
// facts written out here, with no device and no table.  The engine's translation unit under the host emulation
// (-DJFGPU_EMU, as tests/host/build_emu.sh compiles it), in a program of its own (tests/test_part_plan_emu.py builds it
// with -fsanitize=address,undefined and runs it as a plain process).  Three kinds of expectation, none from the plan code:
//   rows of GPU tests  what tests/test_gpu_parity.py asserts from the engine's counters at 2^33 / 2^34 slots, n_cu = 256
//   the kGranMaxB rule  8- and 16-byte items with b2 = 11 take the exact P2 whatever JFGPU_P2_SINGLE says
//   recorded rows      tests/host/plan_cases.txt: facts and decisions the code printed BEFORE it was split into plan and
//                      executor (profiles/flush_plan_parent_print.txt is the print), one line a decision
// Prints one line per case and "plan_check: ok".
#include "../../jellyfish_amd/csrc/jfgpu.hip"

#include <fstream>
#include <map>
#include <set>
#include <sstream>

namespace {

int g_failed = 0;
std::set<std::string> g_arms;
void arm(const std::string& a) { g_arms.insert(a); }

#define EXPECT(cond, what)                                                                       \
  do {                                                                                           \
    if(!(cond)) { printf("plan_check: FAILED %s: %s (%s:%d)\n", (what).c_str(), #cond, __FILE__, __LINE__); ++g_failed; } \
  } while(0)

// ---- facts of the metric's geometries: k = 21, canonical, 2^lsize 4-byte slots, tiles of 2^13 slots, 256 CUs --------
PartFacts metric_facts(uint32_t lsize, uint32_t item_bytes = 4) {
  PartFacts f;
  const uint32_t bits = lsize - 13;
  f.pg.b2 = std::min<uint32_t>(11, (bits + 1) / 2); f.pg.b1 = bits - f.pg.b2;
  f.pg.rest_shift = lsize - f.pg.b1; f.pg.item_bits = f.pg.rest_shift + (42 - lsize);
  f.item_bytes = item_bytes; f.slot32 = item_bytes == 4; f.mode = MODE_PARTITIONED; f.n_cu = 256; f.g1 = 512; f.n_tiles = 1ull << bits;
  f.wide = item_bytes == 16;
  f.nbytes = 6; f.canonical = true; f.lsize_g = f.lsize_l = lsize; f.tile_bits = 13; f.tag_bits = 8;
  f.ws_cap = (size_t)96 << 30; f.ws_used = (size_t)4 << 30;
  return f;
}

std::string kinds_of(const PartFacts& f, const FlushPlan& p, const uint64_t* bt, bool all_granule, bool* tile_dense) {
  std::string s;
  *tile_dense = false;
  for(uint32_t g = 0; g < p.n_groups; ++g) {
    const GroupPlan q = group_plan(f, p, g, bt, all_granule);
    s += q.p2 == kP2Roles ? 'R' : q.p2 == kP2SharedRing ? 'S' : q.p2 == kP2Sort ? 's' : 'X';
    *tile_dense = *tile_dense || q.tile_dense;
  }
  return s;
}

void gpu_test_rows() {
  const uint64_t batch = 1100000ull * 130;                 // 143 M k-mers: 1.1 M reads of 150 bases
  const uint32_t combos[3][2] = {{33, 1}, {34, 1}, {34, 3}};     // (lsize, JFGPU_P2_RING) of test_ring_p2_kernels_at_the_geometries_that_use_them
  for(const auto& combo : combos)
      for(uint32_t want_groups : {1u, 2u}) {               // (room for every region at once; room for half of them: two groups)
        const uint32_t lsize = combo[0]; const int ring = (int)combo[1];
        PartFacts f = metric_facts(lsize);
        f.tun.p2_ring = ring; if(ring == 3) f.tun.p2_single = 2;
        // the regions of a flush are 2 GB at 2^33 slots (2^19 pairs of tiles, 1024 items each) and 3.25 GB at 2^34 (2^20, 832 each)
        const size_t beside_p1 = want_groups == 1 ? (size_t)8 << 30 : lsize == 33 ? (size_t)3 << 29 : (size_t)5 << 29;
        const std::string what = "ring geometries: lsize " + std::to_string(lsize) + ", p2_ring " + std::to_string(ring) + ", " + std::to_string(want_groups) + " group(s)";
        const P1Plan p1 = p1_plan(f, false, 1100000ull * 151, 0, 1100000ll * 151, PendingSum{});
        EXPECT(p1.kind == kP1Ring && !p1.refuse && !p1.flush && p1.gran_cap > 0, what);          // c["p1_ring"] >= 2 and c["p1_other"] == 0
        EXPECT((p1.targs == TArgs{0, 6, 1}) && p1.grid == 256 && p1.lds == 1024 * 128 + 128, what);
        std::vector<uint64_t> bt(1u << f.pg.b1, batch >> f.pg.b1);
        const uint64_t total = (batch >> f.pg.b1) << f.pg.b1;
        f.ws_used = p1.arena; f.ws_cap = p1.arena + beside_p1;
        const FlushPlan p = flush_plan(f, total, bt.data(), 1, true, FlushAllow{});
        bool dense = false;
        const std::string kinds = kinds_of(f, p, bt.data(), true, &dense);
        EXPECT(p.route == kRouteTwoLevel && p.pair && p.cap2 > 0 && !p.one_off, what);
        EXPECT(p.n_groups == want_groups && p.share == (p.n_groups > 1), what);
        EXPECT(kinds == std::string(p.n_groups, ring == 1 ? 'R' : 'S'), what);                     // c["p2_roles" | "p2_ring"] >= 2, no sort, no exact
        EXPECT(dense == (ring == 1), what);                                                        // tests/test_gpu_tile_dense.py: c["tile_dense"]
        printf("plan_check: %-64s P1 ring, P2 %s, tile dense %d\n", what.c_str(), kinds.c_str(), (int)dense);
        arm(ring == 1 ? "gpu_rows_roles" : "gpu_rows_shared_ring");
      }
  // one exact batch beside two granule batches (test_all_ones_item_of_an_exact_batch_..., 2^34 slots)
  for(int ring : {1, 3}) {
    PartFacts f = metric_facts(34);
    f.canonical = false; f.tun.p2_ring = ring; if(ring == 3) f.tun.p2_single = 2;
    std::vector<uint64_t> bt(1024, 2 * batch >> 10);
    bt[5] += 1;
    const uint64_t total = ((2 * batch >> 10) << 10) + 1;
    bool dense = false;
    const std::string what = "exact batch beside granule batches, p2_ring " + std::to_string(ring);
    const FlushPlan p = flush_plan(f, total, bt.data(), 3, false, FlushAllow{});
    const std::string kinds = kinds_of(f, p, bt.data(), false, &dense);
    EXPECT(p.route == kRouteTwoLevel && p.cap2 > 0, what);
    EXPECT(kinds == (ring == 1 ? "R" : "s"), what);
    const std::string again = kinds_of(f, p, bt.data(), true, &dense);     // the same flush without the exact batch takes a ring kernel either way
    EXPECT(again == (ring == 1 ? "R" : "S"), what);
    printf("plan_check: %-64s P2 %s, all granule %s\n", what.c_str(), kinds.c_str(), again.c_str());
    arm("gpu_rows_exact_batch");
  }
}

// 8- and 16-byte items with b2 = 11 (2^34 slots and more): more destinations per bucket than the single-pass kernel places
// (kGranMaxB): exact P2, cap2 = 0, whatever JFGPU_P2_SINGLE says.  4-byte items there are routed to pairs: 1024, single pass.
void gran_max_rows() {
  for(uint32_t item : {4u, 8u, 16u})
    for(uint32_t lsize : {34u, 35u})
      for(int single : {1, 2}) {
        PartFacts f = metric_facts(lsize, item);
        f.tun.p2_single = single;
        const std::string what = "b2 = 11, " + std::to_string(item) + "-byte items, 2^" + std::to_string(lsize) + " slots, p2_single " + std::to_string(single);
        EXPECT(f.pg.b2 == 11, what);
        std::vector<uint64_t> bt(1u << f.pg.b1, (uint64_t)1 << 21);
        const uint64_t total = (uint64_t)1 << (21 + f.pg.b1);
        const FlushPlan p = flush_plan(f, total, bt.data(), 2, true, FlushAllow{});
        bool dense = false;
        const std::string kinds = kinds_of(f, p, bt.data(), true, &dense);
        EXPECT(p.route == kRouteTwoLevel, what);
        if(item == 4) { EXPECT(p.pair && p.b2e == 10 && p.n_dest == f.n_tiles / 2 && p.cap2 > 0 && kinds.find('X') == std::string::npos, what); }
        else { EXPECT(!p.pair && p.b2e == 11 && p.cap2 == 0 && kinds == std::string(p.n_groups, 'X'), what); }
        printf("plan_check: %-64s cap2 %u, P2 %s\n", what.c_str(), p.cap2, kinds.c_str());
        arm(item == 4 ? "gran_max_pairs_single_pass" : "gran_max_exact");
      }
  // An arena with no room for the single pass's regions, in any number of groups: the flush falls to the exact P2 (and, with
  // no room for its temporaries either, to one-off blocks).  2^33 slots, 143 M items, 1 MiB free behind what is pending.
  {
    PartFacts f = metric_facts(33);
    f.ws_used = (size_t)1 << 30; f.ws_cap = f.ws_used + ((size_t)1 << 20);
    std::vector<uint64_t> bt(1024, 139648);
    const FlushPlan p = flush_plan(f, 1024 * 139648ull, bt.data(), 1, true, FlushAllow{});
    bool dense = false;
    const std::string what = "arena too small for the regions", kinds = kinds_of(f, p, bt.data(), true, &dense);
    EXPECT(p.route == kRouteTwoLevel && p.pair && p.cap2 == 0 && p.n_groups == 1 && !p.share && p.one_off && kinds == "X" && p.tmp_items == 1024 * 139648ull, what);
    printf("plan_check: %-64s cap2 %u, P2 %s, one-off %d\n", what.c_str(), p.cap2, kinds.c_str(), (int)p.one_off);
    arm("flush_arena_too_small_for_regions");
  }
  // granule_cap: a batch whose regions would pass 0xFFFF0000 items takes the exact scheme
  PartFacts f = metric_facts(34);
  f.ws_cap = (size_t)1 << 46;
  const P1Plan big = p1_plan(f, false, (uint64_t)5 << 40, 0, (int64_t)5 << 40, PendingSum{});
  EXPECT(big.gran_cap == 0 && big.kind == kP1ExactSorted, std::string("granule_cap above 0xFFFF0000"));
  const P1Plan fits = p1_plan(f, false, (uint64_t)3 << 40, 0, (int64_t)3 << 40, PendingSum{});
  EXPECT(fits.gran_cap > 0xC0000000u && fits.kind == kP1Ring, std::string("granule_cap below 0xFFFF0000"));
  printf("plan_check: granule_cap of 5 * 2^40 items: %u, of 3 * 2^40: %u\n", big.gran_cap, fits.gran_cap);
  arm("granule_cap_too_large");
}

// ---- recorded rows -------------------------------------------------------------------------------------------------
typedef std::map<std::string, std::string> Row;
uint64_t U(const Row& r, const char* k) { auto it = r.find(k); if(it == r.end()) { printf("plan_check: row lacks %s\n", k); exit(2); } return strtoull(it->second.c_str(), nullptr, 10); }
long long I(const Row& r, const char* k) { auto it = r.find(k); if(it == r.end()) { printf("plan_check: row lacks %s\n", k); exit(2); } return strtoll(it->second.c_str(), nullptr, 10); }
double D(const Row& r, const char* k) { auto it = r.find(k); if(it == r.end()) { printf("plan_check: row lacks %s\n", k); exit(2); } return strtod(it->second.c_str(), nullptr); }
bool has(const Row& r, const char* k) { return r.count(k) != 0; }

PartFacts facts_of(const Row& r) {
  PartFacts f;
  f.pg.b1 = (uint32_t)U(r, "b1"); f.pg.b2 = (uint32_t)U(r, "b2");
  f.item_bytes = (uint32_t)U(r, "item"); f.slot32 = U(r, "slot32"); f.mode = (int)I(r, "mode"); f.n_cu = (int)I(r, "n_cu"); f.g1 = (int)I(r, "g1"); f.n_tiles = U(r, "n_tiles");
  f.returning = U(r, "rt"); f.wide = U(r, "wide"); f.filter = U(r, "filter"); f.filter_kind = (int)I(r, "fkind");
  f.nbytes = (uint32_t)U(r, "nbytes"); f.hash_xs = U(r, "xs"); f.canonical = U(r, "canon"); f.lsize_g = (uint32_t)U(r, "lsize_g"); f.lsize_l = (uint32_t)U(r, "lsize_l");
  f.tile_bits = (uint32_t)U(r, "tile_bits"); f.tag_bits = (uint32_t)U(r, "tag_bits");
  f.pg.rest_shift = f.lsize_l - f.pg.b1;
  f.items_per_byte = D(r, "ipb"); f.ws_cap = U(r, "ws_cap"); f.ws_used = U(r, "ws_used"); f.reserved_input = U(r, "reserved");
  f.tun.p1_single = (int)I(r, "p1_single"); f.tun.p1_slack = D(r, "p1_slack"); f.tun.flush_groups = (int)I(r, "flush_groups"); f.tun.tile_pair = U(r, "tile_pair");
  f.tun.p2_single = (int)I(r, "p2_single"); f.tun.p2_cap = (uint32_t)U(r, "p2_cap"); f.tun.p2_slack = D(r, "p2_slack"); f.tun.tile_adapt = (int)I(r, "tile_adapt");
  f.tun.flush_share = (uint32_t)U(r, "flush_share"); f.tun.p2_ring = (int)I(r, "p2_ring"); f.tun.p2_depth = (int)I(r, "p2_depth");
  return f;
}

const char* p1_kind_name(int k) {
  switch(k) {
  case kP1Ring: return "ring"; case kP1KeysGranule: return "keys_granule"; case kP1Granule64: return "granule64"; case kP1WideGranule: return "wide";
  case kP1ExactSorted: return "exact_sorted"; case kP1ExactKeysSorted: return "exact_keys_sorted"; default: return "exact_plain";
  }
}

void check_p1_row(const Row& r, const std::string& what) {
  const PartFacts f = facts_of(r);
  const P1Plan p = p1_plan(f, U(r, "from_keys"), U(r, "max_items"), I(r, "lo"), I(r, "hi"), PendingSum{(size_t)U(r, "pend_n"), U(r, "pend_in")});
  std::string got;
  if(!has(r, "refuse")) {                      // the batch list was full
    EXPECT(p.flush == kFlushSegments && I(r, "flush") == 1, what);
    got = "flush first: batch list full"; arm("p1_flush_segments");
  } else if(U(r, "refuse")) {
    EXPECT(p.refuse && p.gran_cap == U(r, "gcap"), what);
    got = std::string("refused: ") + (f.wide ? "two-word keys" : "one-pass filter"); arm(f.wide ? "p1_refuse_wide" : "p1_refuse_filter");
  } else {
    static const char* why[] = {"", "", "p1_flush_wide_share", "p1_flush_even", "p1_flush_arena_full"};
    EXPECT(!p.refuse && p.flush == I(r, "flush") && p.gran_cap == U(r, "gcap") && p.bytes == U(r, "bytes") && p.arena == U(r, "arena"), what);
    EXPECT(r.at("kind") == p1_kind_name(p.kind), what);
    if(p.flush) arm(why[p.flush]);
    arm(std::string("p1_") + p1_kind_name(p.kind));
    if(!p.gran_cap && f.pg.b2 && f.pg.b1 <= 10 && f.tun.p1_single < 0 && !(f.item_bytes == 8 && U(r, "from_keys"))) arm("granule_cap_small_batch");
    got = std::string(p1_kind_name(p.kind)) + ", regions of " + std::to_string(p.gran_cap) + ", flush first " + std::to_string(p.flush);
  }
  printf("plan_check: %-40s %s\n", what.c_str(), got.c_str());
}

void check_flush_row(const Row& r, const std::string& what) {
  const PartFacts f = facts_of(r);
  std::vector<uint64_t> bt;
  { std::stringstream ss(r.at("bucket_tot")); std::string run;
    while(std::getline(ss, run, ',')) { const size_t star = run.find('*'); bt.insert(bt.end(), strtoull(run.c_str(), nullptr, 10), strtoull(run.c_str() + star + 1, nullptr, 10)); } }
  EXPECT(bt.size() == (size_t)1 << f.pg.b1, what);
  if(bt.size() != (size_t)1 << f.pg.b1) return;
  const bool all_granule = U(r, "all_granule");
  const FlushPlan p = flush_plan(f, U(r, "total"), bt.data(), U(r, "nbatch"), all_granule, FlushAllow{});
  static const char* routes[] = {"nothing", "direct", "single_level", "two_level"};
  EXPECT(r.at("route") == routes[p.route], what);
  std::string got = routes[p.route];
  if(p.route == kRouteTwoLevel && r.at("route") == "two_level") {
    bool dense = false;
    const std::string kinds = kinds_of(f, p, bt.data(), all_granule, &dense);
    EXPECT(p.pair == (bool)U(r, "pair") && p.cap2 == U(r, "cap2") && p.n_dest == U(r, "n_dest") && p.b2e == U(r, "b2e") && p.p2_tag_bits == U(r, "p2_tag_bits"), what);
    EXPECT(p.n_groups == U(r, "n_groups") && p.share == (bool)U(r, "share") && p.two_streams == (bool)U(r, "two_streams") && p.one_off == (bool)U(r, "one_off"), what);
    EXPECT(p.cap2 || p.tmp_items == U(r, "tmp_items"), what);
    EXPECT(kinds == r.at("kinds") && dense == (bool)U(r, "tile_dense"), what);
    EXPECT(!p.no_memory, what);
    got += ", pairs " + std::to_string(p.pair) + ", cap2 " + std::to_string(p.cap2) + ", " + std::to_string(p.n_groups) + " group(s) " + kinds + (p.share ? " sharing" : "") + (p.two_streams ? " on two streams" : "") + (p.one_off ? ", one-off blocks" : "");
    const std::string w = std::to_string(f.item_bytes);
    if(kinds.find('s') != std::string::npos) arm("flush_sort_" + w);
    if(kinds.find('X') != std::string::npos) arm(p.pair ? "flush_exact_pair" : "flush_exact_tiles");
    if(p.share) arm(p.cap2 ? "flush_share_single_pass" : "flush_share_exact");
    if(f.tun.flush_share && p.share) arm(p.cap2 ? "flush_share_forced_single_pass" : "flush_share_forced_exact");
    if(f.tun.p2_cap && p.cap2 == f.tun.p2_cap) arm("flush_p2_cap");
    if(p.two_streams) arm("flush_two_streams");
    if(!f.tun.tile_pair && f.item_bytes == 4 && f.slot32) arm("flush_tile_pair_0");
    if(!p.cap2 && p.one_off) arm("flush_arena_too_small_for_tmp");
    if(p.cap2 && p.one_off) arm("flush_single_pass_one_off");
    // what was struck stays struck: without the one-off blocks the forced single pass is the exact P2, and the exact P2 fails
    FlushAllow none; none.single_one_off = none.exact_one_off = false;
    const FlushPlan q = flush_plan(f, U(r, "total"), bt.data(), U(r, "nbatch"), all_granule, none);
    if(p.one_off) { EXPECT(q.cap2 == 0 && (q.no_memory || !q.one_off), what); }
    else { EXPECT(q.cap2 == p.cap2 && q.n_groups == p.n_groups && !q.no_memory, what); }
  } else if(p.route == kRouteDirect) arm("flush_items_direct");
  else if(p.route == kRouteSingleLevel) arm(f.wide ? "flush_single_level_two_word" : "flush_single_level_one_word");
  printf("plan_check: %-40s %s\n", what.c_str(), got.c_str());
}

int recorded_rows(const char* path) {
  std::ifstream in(path);
  if(!in) { printf("plan_check: cannot read %s\n", path); return 2; }
  std::string line;
  int n = 0;
  while(std::getline(in, line)) {
    if(line.empty() || line[0] == '#') continue;
    std::stringstream ss(line);
    std::string w, tag, kind;
    ss >> tag >> kind;
    Row r;
    while(ss >> w) { const size_t eq = w.find('='); if(eq != std::string::npos && w != "=>") r[w.substr(0, eq)] = w.substr(eq + 1); }
    const std::string what = "recorded row " + std::to_string(++n) + " (" + kind + ")";
    if(kind == "p1") check_p1_row(r, what); else check_flush_row(r, what);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  gpu_test_rows();
  gran_max_rows();
  if(const int rc = recorded_rows(argc > 1 ? argv[1] : "tests/host/plan_cases.txt")) return rc;
  for(const std::string& a : g_arms) printf("plan_check: arm %s\n", a.c_str());
  if(g_failed) { printf("plan_check: %d expectations FAILED\n", g_failed); return 1; }
  printf("plan_check: ok\n");
  return 0;
}
