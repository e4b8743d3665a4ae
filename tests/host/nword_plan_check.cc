// tests/host/nword_plan_check.cc -- TEST-ONLY: what the partitioned insert decides for keys of three and four words, with no
// device: the partition geometry of every legal table (host_partition.inl: part_geom_init) and the plans of part_plan.inl on
// facts written out here.  The engine's translation unit under the host emulation (-DJFGPU_EMU), in a program of its own
// (tests/test_nword_part_emu.py builds it with -fsanitize=address,undefined and runs it as a plain process).
//   geometry   every k in 65 .. 128 and every lsize from nword_min_lsize(k) to 48: b1 / b2 by the rule written out here, 32-byte
//              items of 2k - b1 bits, the path exactly up to 2^32 slots, and no geometry whose largest item is the hole
//   plans      which kernels are named for a batch and a flush, and that every named instantiation exists (its address is
//              taken here: a name without a kernel does not link)
// Prints one line per group of cases and "nword_plan_check: ok".
#include "../../jellyfish_amd/csrc/jfgpu.hip"

namespace {

int g_failed = 0;
#define EXPECT(cond, what)                                                                       \
  do {                                                                                           \
    if(!(cond)) { printf("nword_plan_check: FAILED %s: %s (%s:%d)\n", std::string(what).c_str(), #cond, __FILE__, __LINE__); ++g_failed; } \
  } while(0)

uint32_t popcount256(const K256& v) { uint32_t n = 0; for(int i = 0; i < 4; ++i) n += (uint32_t)__builtin_popcountll(v.w[i]); return n; }

void geometries() {
  uint32_t seen = 0, with_path = 0, two_level = 0;
  for(uint32_t k = 65; k <= 128; ++k)
    for(uint32_t lsize = nword_min_lsize(k); lsize <= 48; ++lsize) {
      const std::string what = "k " + std::to_string(k) + ", lsize " + std::to_string(lsize);
      jfgpu_table t;
      t.nword = true;
      EXPECT(nword_geom_init(t.nt.N, k, lsize, 1), what);
      t.g = t.nt.N.g;
      part_geom_init(&t);
      ++seen;
      // the rule, written out: one level up to 2^10 tiles, then b2 = min(11, ceil(bits / 2)); b1 <= 10
      const uint32_t bits = lsize - kNTileBits;
      const uint32_t b2 = bits <= 10 ? 0 : std::min<uint32_t>(11, (bits + 1) / 2), b1 = bits - b2;
      EXPECT(t.part_ok == (lsize <= 32), what);
      EXPECT(!t.item32 && !t.item128, what);
      if(!t.part_ok) { EXPECT(b1 > 10, what); continue; }
      ++with_path; two_level += b2 != 0;
      EXPECT(t.item256 && item_size(&t) == 32, what);
      EXPECT(t.pg.b1 == b1 && t.pg.b2 == b2 && b1 <= 10 && b2 <= 11, what);
      EXPECT(t.pg.rest_shift == lsize - b1 && t.pg.item_bits == 2 * k - b1, what);
      EXPECT(t.pg.item_bits < 256, what);                                   // bit 255 is clear: an item is never the hole
      if(k == 128) EXPECT(lsize >= 31 && b1 >= 1, what);
      // the largest item this geometry makes: every key bit and every position bit set
      const u256 top = make_item_nword(t.nt.N, t.pg, t.nt.N.key_mask, t.g.local_mask);
      EXPECT(!(top == ~u256(0)), what);
      EXPECT(popcount256(top.v) == t.pg.item_bits && k256_shr(top.v, t.pg.item_bits - 1).w[0] == 1, what);
      // ... and what the kernels read back from it: the P2 sub-bucket above tag_full, the tag below
      EXPECT((uint32_t)(top >> t.nt.N.tag_full) == (1u << b2) - 1, what);
      EXPECT(t.nt.N.tag_full + b2 == t.pg.item_bits, what);
    }
  printf("nword_plan_check: %u geometries, %u with the partitioned path (%u in two levels), none whose largest item is the hole\n", seen, with_path, two_level);
  EXPECT(seen > 2000 && with_path > 1000 && two_level > 500, std::string("geometry counts"));
}

PartFacts nword_facts(uint32_t k, uint32_t lsize, int mode, bool returning) {
  jfgpu_table t;
  t.nword = true;
  nword_geom_init(t.nt.N, k, lsize, 1);
  t.g = t.nt.N.g;
  part_geom_init(&t);
  PartFacts f;
  f.pg = t.pg; f.item_bytes = 32; f.mode = mode; f.n_cu = 256; f.g1 = 512; f.n_tiles = 1ull << (lsize - kNTileBits);
  f.returning = returning; f.nword = true; f.nbytes = t.g.nbytes; f.canonical = true; f.lsize_g = f.lsize_l = lsize; f.tile_bits = kNTileBits;
  f.tag_bits = t.nt.N.tag_full;
  f.ws_cap = (size_t)64 << 30;
  return f;
}

void plans() {
  // a kernel the plans may name, by its template arguments: taking the address instantiates it
  const void* p1[2] = {(const void*)p1_nword_granule_kernel<false>, (const void*)p1_nword_granule_kernel<true>};
  const void* tn[2] = {(const void*)tile_insert_nword_kernel<false>, (const void*)tile_insert_nword_kernel<true>};
  const void* dn[2] = {(const void*)items_direct_nword_kernel<false>, (const void*)items_direct_nword_kernel<true>};
  const void* p2[3] = {(const void*)p2_kernel<u256, false>, (const void*)scan_matrix_kernel, (const void*)p2_scatter_sorted_kernel<u256, kP2NWordPer>};
  for(const void* q : p1) EXPECT(q != nullptr, std::string("P1n"));
  for(const void* q : tn) EXPECT(q != nullptr, std::string("Tn"));
  for(const void* q : dn) EXPECT(q != nullptr, std::string("direct"));
  for(const void* q : p2) EXPECT(q != nullptr, std::string("P2"));
  const uint64_t batch = 64ull << 20;
  for(uint32_t lsize : {12u, 21u, 22u, 31u, 32u})
    for(int rt : {0, 1}) {
      const uint32_t k = lsize >= 30 ? 128 : 100;
      const std::string what = "k " + std::to_string(k) + ", lsize " + std::to_string(lsize) + ", returning " + std::to_string(rt);
      PartFacts f = nword_facts(k, lsize, MODE_PARTITIONED, rt != 0);
      const P1Plan p = p1_plan(f, false, batch, 0, (int64_t)batch, PendingSum{});
      EXPECT(!p.refuse && !p.flush && p.kind == kP1NWordGranule && p.gran_cap > 0 && p.gran_cap % kGran == 0, what);
      EXPECT((p.targs == TArgs{rt}) && (pick<Inst<1>, Inst<0>>(p.targs, [](auto) {})), what);
      EXPECT(p.lds == (size_t)kNChunk * 34 + (size_t)f.nbytes * 2048 && f.nbytes == (2 * k + 7) / 8 && p.lds + sizeof(GranuleLds) + 2 * (kPBlock + 8) * 4 <= 160 * 1024, what);   // items, bucket ids, byte tables, the sort's state, the staged codes
      EXPECT(p.bytes == ((size_t)p.gran_cap << f.pg.b1) * 32 && p.bytes % 128 == 0 && p.grid == 512, what);
      // encoded keys and a filtered pass stay on the direct kernel
      EXPECT(p1_plan(f, true, 1 << 20, 0, 1 << 20, PendingSum{}).refuse, what);
      PartFacts ff = f; ff.filter = true;
      EXPECT(p1_plan(ff, false, batch, 0, (int64_t)batch, PendingSum{}).refuse, what);
      // the flush
      const uint32_t nb1 = 1u << f.pg.b1;
      std::vector<uint64_t> bt(nb1, batch / nb1);
      for(int single : {1, 2}) {
        f.tun.p2_single = single;
        const FlushPlan q = flush_plan(f, batch / nb1 * nb1, bt.data(), 2, true, FlushAllow{});
        if(f.pg.b2 == 0) { EXPECT(q.route == kRouteSingleLevel, what); continue; }
        EXPECT(q.route == kRouteTwoLevel && q.cap2 == 0 && !q.pair && q.b2e == f.pg.b2 && q.p2_tag_bits == f.tag_bits, what);    // 32-byte items: the exact P2 only
        EXPECT(q.n_dest == f.n_tiles && q.block_bytes[2] == q.tmp_items * 32, what);
        for(uint32_t g = 0; g < q.n_groups; ++g) {
          const GroupPlan gp = group_plan(f, q, g, bt.data(), true);
          EXPECT(gp.p2 == kP2Exact && (gp.p2_targs == TArgs{kP2NWordPer}) && gp.grid_x == kG2Exact && gp.sample == 0, what);
          EXPECT(gp.lds == (size_t)kPBlock * kP2NWordPer * 32 && gp.lds + 3 * kMaxBuckets * 4 + 64 <= 160 * 1024, what);
        }
      }
      // nothing pending: nothing to do; auto mode with a handful of items: straight from the items
      EXPECT(flush_plan(f, 0, bt.data(), 0, true, FlushAllow{}).route == kRouteNothing, what);
      PartFacts fa = f; fa.mode = MODE_AUTO;
      EXPECT(flush_plan(fa, 100, bt.data(), 1, true, FlushAllow{}).route == kRouteDirect, what);
    }
  printf("nword_plan_check: plans name p1_nword_granule_kernel, the exact P2 on u256 and tile_insert_nword_kernel; every instantiation exists\n");
}

}  // namespace

int main() {
  geometries();
  plans();
  if(g_failed) { printf("nword_plan_check: %d expectation(s) failed\n", g_failed); return 1; }
  printf("nword_plan_check: ok\n");
  return 0;
}
