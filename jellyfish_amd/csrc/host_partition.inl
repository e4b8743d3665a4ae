// jellyfish_amd/csrc/host_partition.inl -- host orchestration of the partitioned insert path (kernels_part.hip.hpp):
// workspace arena, P1 ingestion of a batch, the flush (P2 + tile insert).  Included by jfgpu.hip inside its
// anonymous namespace.  What lives across calls (the arena, M1 / M2, the straggler lists, the second stream) is a member of
// jfgpu_table and owned by it; what a flush allocates for itself when the arena has no room is a local DevBuf (hip_own.hpp).
// Every choice -- which kernel, how many groups, which blocks of the arena -- is made by part_plan.inl's pure functions from
// a PartFacts; part_ingest and part_flush_t gather the facts, ask for the plan and carry it out.
constexpr uint64_t kPartMinBytes = 1u << 20;   // AUTO: smaller device batches take the direct kernel

// Keys of three and four words, AUTO: the partitioned path exactly where profiles/nword_part_rate.txt shows it faster than the
// direct kernel by more than the spread of five runs -- one batch of 1 GiB of reads, k = 65 / 96 / 100, 2^30 slots (a flush
// streams every tile that gets an item, and a batch's bucket regions hold a stranded reservation per workgroup: smaller
// batches lose, as does k = 128 in its 2^31 slots).  k between 100 and 128 and larger tables were not measured: never there.
// JFGPU_MODE=partitioned / jfgpu_set_mode(t, 2) take the path for every batch.
constexpr uint64_t kNWordPartMinBytes = 1ull << 30;
constexpr uint32_t kNWordPartMaxK = 100, kNWordPartMaxLsize = 30;
bool nword_auto_partitioned(const TableGeom& g, size_t nbytes) { return nbytes >= kNWordPartMinBytes && g.k <= kNWordPartMaxK && g.lsize_l <= kNWordPartMaxLsize; }

void part_geom_init(jfgpu_table* t) {
  const uint32_t bits = t->g.lsize_l - t->g.tile_bits;   // tile-index bits to resolve
  t->part_ok = false; t->item32 = false; t->item128 = false; t->item256 = false;
  if(!t->nword && t->g.tile_bits < kMaxTileBits) return;  // tiny table: one partial tile (keys of three and four words: tiles of 2^11 slots, all whole)
  uint32_t b1, b2;
  const uint32_t one_level = t->wide || t->nword ? 10 : 11;   // keys of two and more words only have the single-pass P1 (<= 1024 buckets)
  if(bits <= one_level) { b1 = bits; b2 = 0; }
  else { b2 = std::min<uint32_t>(11, (bits + 1) / 2); b1 = bits - b2; }
  if(b1 > one_level) return;
  t->pg.b1 = b1; t->pg.b2 = b2;
  t->pg.rest_shift = t->g.lsize_l - b1;
  t->pg.item_bits = t->pg.rest_shift + t->g.rem_bits;
  if(t->wide) { t->item128 = true; t->part_ok = t->pg.item_bits <= 128; return; }
  // 256-bit items: all ones is the hole, so an item must never be all ones -- it cannot be while it has fewer than 256 bits
  // (bit 255 is clear).  It has 2k - b1 of them, and k = 128 forces lsize >= 31, hence b1 >= 1: no geometry is refused here
  // today (tests/test_nword_part_emu.py walks them all), but a hole that is an item drops k-mers silently.
  if(t->nword) { t->item256 = true; t->part_ok = t->pg.item_bits < 256; return; }
  if(t->pg.item_bits > 64) return;
  t->item32 = t->pg.item_bits <= 32;
  t->part_ok = true;
}

size_t item_size(const jfgpu_table* t) { return t->item256 ? 32 : t->item128 ? 16 : t->item32 ? 4 : 8; }

// what the plans may know of a table (part_plan.inl)
PartFacts part_facts(const jfgpu_table* t) {
  PartFacts f;
  const DevBloom& bloom = table_bloom(t);
  f.pg = t->pg; f.item_bytes = (uint32_t)item_size(t); f.slot32 = t->g.slot32; f.mode = t->mode; f.n_cu = t->n_cu; f.g1 = t->g1; f.n_tiles = n_tiles_of(t);
  f.returning = t->returning; f.wide = t->wide; f.nword = t->nword; f.filter = bloom.data != nullptr; f.filter_kind = (int)bloom.kind;
  f.nbytes = t->g.nbytes; f.hash_xs = t->g.hash_xs; f.canonical = t->g.canonical; f.lsize_g = t->g.lsize_g; f.lsize_l = t->g.lsize_l; f.tile_bits = t->g.tile_bits;
  f.tag_bits = t->item256 ? t->nt.N.tag_full : t->item128 ? t->wt.W.tag_full : t->g.tag_bits;
  f.items_per_byte = t->items_per_byte; f.ws_cap = t->ws_cap; f.ws_used = t->ws_used; f.reserved_input = t->reserved_input; f.tun = t->tun;
  return f;
}

// The table's descriptor in device memory, for kernels that leave their hot loop through a real call (item_direct_call):
// refreshed in stream order before every launch that uses it.
int refresh_d_dt(jfgpu_table* t) {
  if(!t->d_dt) { const int rc = t->d_dt.alloc(1); if(rc) return rc; }
  HIP_TRY(hipMemcpyAsync(t->d_dt, &t->dt, sizeof(DevTable), hipMemcpyHostToDevice, t->stream));
  return JFGPU_OK;
}

// Grow the arena to at least `need` bytes.  Only legal while it holds nothing (ws_used == 0).
int ws_grow(jfgpu_table* t, size_t need) {
  if(need <= t->ws_cap) return JFGPU_OK;
  size_t want = std::max(need + need / 8, t->ws_cap * 2);
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipStreamSynchronize(t->stream));
  (void)t->ws.reset(); t->ws_cap = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const size_t keep = (size_t)2 << 30;                      // leave room for the caller's buffers
  if(want + keep > free_b) want = need;
  if(want + keep / 2 > free_b) return -1;
  { const int rc = t->ws.alloc(want); if(rc) return rc; }
  t->ws_cap = want;
  return JFGPU_OK;
}

void* ws_alloc(jfgpu_table* t, size_t bytes) {
  const size_t at = arena_take(t->ws_used, t->ws_cap, bytes);
  return at == kNoBlock ? nullptr : t->ws + at;
}

int no_kernel(const char* what) { return fail(JFGPU_E_UNSUPPORTED, std::string("partition plan names an instantiation that does not exist: ") + what); }

// p1_kernel, the exact scheme's count pass (SC = 0) and plain scatter (SC = 1): <SC, FK, RT, BL, N>
template <typename ITEM>
bool launch_p1(jfgpu_table* t, const TArgs& inst, const uint8_t* base, int64_t lo, int64_t hi, const uint64_t* d_off, void* d_items) {
  return pick<Inst<0, 1, 0, 0, 6>, Inst<0, 1, 0, 0, 7>, Inst<0, 1, 0, 0, 8>, Inst<0, 0, 0, 0, 6>, Inst<0, 0, 0, 0, 7>, Inst<0, 0, 0, 0, 8>,
              Inst<0, 1, 0, 0, 0>, Inst<0, 0, 0, 1, 0>, Inst<0, 0, 0, 0, 0>,
              Inst<1, 1, 1, 0, 0>, Inst<1, 1, 0, 0, 0>, Inst<1, 0, 1, 1, 0>, Inst<1, 0, 0, 1, 0>, Inst<1, 0, 1, 0, 0>, Inst<1, 0, 0, 0, 0>>(inst, [&](auto I) {
    constexpr auto& A = decltype(I)::v;
    hipLaunchKernelGGL((p1_kernel<ITEM, A[0] != 0, A[1] != 0, A[2] != 0, A[3] != 0, A[4]>), dim3(t->g1), dim3(kPBlock), 0, t->stream,
                       t->dt, t->pg, base, lo, hi, t->d_M1, d_off, (ITEM*)d_items);
  });
}

int part_flush(jfgpu_table* t);

// JFGPU_FLUSH_TRACE: how full the blocks' straggler lists of a p2_ring_kernel launch ran (waits for the stream)
int trace_strag_lists(hipStream_t stream, const uint32_t* d_n, uint32_t n_lists, uint32_t list_cap, uint32_t per_bucket, uint32_t bucket0) {
  std::vector<uint32_t> hn(n_lists);
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipMemcpy(hn.data(), d_n, n_lists * sizeof(uint32_t), hipMemcpyDeviceToHost));
  uint64_t sum = 0; uint32_t mx = 0, at_cap = 0, over256 = 0;
  for(uint32_t v : hn) { sum += v; mx = std::max(mx, v); at_cap += v >= list_cap; over256 += v > 256; }
  fprintf(stderr, "[jfgpu flush] P2 ring stragglers: %llu in %u lists, max %u, %u lists > 256, %u lists full\n", (unsigned long long)sum, n_lists, mx, over256, at_cap);
  for(uint32_t l = 0, shown = 0; l < n_lists && shown < 8; ++l)
    if(hn[l] >= list_cap) { fprintf(stderr, "[jfgpu flush]   full list %u (bucket %u, block %u)\n", l, bucket0 + l / per_bucket, l % per_bucket); ++shown; }
  return JFGPU_OK;
}

// Single-pass P2 of one bucket group of 4-byte items through per-destination rings (kP2Roles, kP2SharedRing: part_plan.inl);
// then what did not go through a ring is appended to its region by the straggler kernel, before the regions' bounds are taken.
int launch_p2_rings(jfgpu_table* t, const FlushPlan& p, const GroupPlan& q, const SegList& S1, unsigned int* d_gcur2, uint32_t* out_v) {
  const bool roles = q.p2 == kP2Roles;
  const uint32_t n_lists = roles ? q.nbk : kG2Blocks * q.nbk;
  if(!t->d_strag2 || !t->d_strag2_n || t->strag2_lists < n_lists) {
    t->strag2_lists = 0;
    (void)t->d_strag2.reset(); (void)t->d_strag2_n.reset();
    int rc;
    if((rc = t->d_strag2.alloc((size_t)n_lists * kP2StragPerBlock)) || (rc = t->d_strag2_n.alloc(n_lists))) return rc;
    t->strag2_lists = n_lists;
  }
  const P2RingDirect pd{t->d_dt, t->pg.b2, p.b2e, (int)t->returning};
  unsigned long long* ctr = (unsigned long long*)&t->dt.counters[CTR_DIRECT];
  const dim3 grid(q.grid_x, q.grid_y), block(kPBlock);
  int rc = JFGPU_OK;
  if(roles) {
    ++t->n_p2_roles;
    if(!pick<Inst<2, 1>, Inst<2, 2>, Inst<2, 3>, Inst<1, 1>, Inst<1, 2>, Inst<1, 3>>(q.p2_targs, [&](auto I) {
         constexpr auto& A = decltype(I)::v;
         rc = launch_lds(p2_ring_roles_kernel<uint32_t, A[0], P2RingDirect, A[1]>, grid, block, q.lds, t->stream, pd, p.b2e, p.p2_tag_bits, S1, p.cap2, d_gcur2, out_v, q.b0,
                         t->d_strag2.get(), t->d_strag2_n.get(), ctr);
       })) return no_kernel("p2_ring_roles_kernel");
  } else {
    ++t->n_p2_ring;
    rc = launch_lds(p2_ring_kernel<P2RingDirect>, grid, block, q.lds, t->stream, pd, p.b2e, p.p2_tag_bits, S1, p.cap2, d_gcur2, d_gcur2 + p.n_dest,
                    out_v, q.b0, (unsigned long long*)nullptr, t->d_strag2.get(), t->d_strag2_n.get(), ctr);
  }
  if(rc) return rc;
  hipLaunchKernelGGL((p1_stragglers_kernel<uint32_t, P2RingDirect>), dim3(t->n_cu), dim3(256), 0, t->stream, pd, ctr, (const uint64_t*)t->d_strag2, (const uint32_t*)t->d_strag2_n,
                     n_lists, p.cap2, d_gcur2, (unsigned long long*)nullptr, out_v, kP2StragPerBlock);
  if(t->tun.flush_trace) return trace_strag_lists(t->stream, t->d_strag2_n, n_lists, kP2StragPerBlock, roles ? 1 : kG2Blocks, q.b0);
  return JFGPU_OK;
}

// per-workgroup straggler lists of the ring P1 kernels (kernels_p1ring.hip.hpp), allocated at first use
int ensure_strag(jfgpu_table* t) {
  if(t->d_strag && t->d_strag_n) return JFGPU_OK;
  const size_t words = Ring<uint32_t>::kWords;
  int rc;
  if((rc = t->d_strag.alloc((size_t)t->n_cu * kStragPerBlock * words)) || (rc = t->d_strag_n.alloc((size_t)t->n_cu))) return rc;
  return JFGPU_OK;
}

// count --bc: the cache of admitted k-mers (kernels_bloom.hip.hpp: bloom_cache_hit / _insert), 2^log2 two-way sets of
// 8-byte words, as much as the device has room for.  No room: the pass goes on without (state -1).
int bloom_cache_enable(jfgpu_table* t) {
  t->bcache_state = -1;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  uint32_t lg = t->tun.bloom_cache_log2;
  while(lg > 16 && ((size_t)16 << lg) + ((size_t)6 << 30) > free_b) --lg;
  if(((size_t)16 << lg) + ((size_t)1 << 30) > free_b && lg > 16) return JFGPU_OK;
  if(!t->d_bcache.try_alloc((size_t)2 << lg)) { (void)hipGetLastError(); return JFGPU_OK; }
  HIP_TRY(hipMemsetAsync(t->d_bcache, 0, (size_t)16 << lg, t->stream));
  t->dt.bloom.cache = t->d_bcache; t->dt.bloom.cache_mask = ((uint64_t)1 << lg) - 1;
  t->bcache_state = 1;
  if(t->tun.flush_trace) fprintf(stderr, "[jfgpu] count --bc: cache of admitted k-mers on, 2^%u sets (%.1f GB)\n", lg, (double)((size_t)16 << lg) / 1e9);
  return JFGPU_OK;
}
// Undecided and batches of a filtered pass are pending: how many of their windows did the counter admit?  One wait for
// the P1 launches already enqueued, once per attachment.  Uniform reads admit next to nothing (a cache would add a read
// per window: off); high-coverage reads admit most windows, each true k-mer dozens of times (on).
int bloom_cache_decide(jfgpu_table* t) {
  const uint32_t nb1 = 1u << t->pg.b1;
  std::vector<uint64_t> tot(nb1);
  uint64_t ctr[CTR_COUNT], admitted = 0;
  bool all_known = true;
  for(const PendingBatch& pb : t->pending) {
    if(!pb.gran_cap) { all_known = false; continue; }
    HIP_TRY(hipMemcpyAsync(tot.data(), pb.tot, nb1 * sizeof(uint64_t), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    for(uint64_t v : tot) admitted += v;
  }
  HIP_TRY(hipMemcpyAsync(ctr, t->dt.counters, sizeof(ctr), hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  const uint64_t windows = ctr[CTR_MERS] >= t->mers_seen ? ctr[CTR_MERS] - t->mers_seen : 0;
  if(windows < (1u << 20) || !all_known) return JFGPU_OK;             // too little to tell: ask again at the next batch
  if(admitted * 100 < windows * 15) { t->bcache_state = -1; return JFGPU_OK; }
  return bloom_cache_enable(t);
}

// What the next batch's plan reads and only the device knows, while batches are pending.
int refresh_estimates(jfgpu_table* t, bool from_keys) {
  if(t->pending.empty() || from_keys) return JFGPU_OK;
  // 16- and 32-byte items: before the first flush the bucket regions are sized for one item per input byte; reads of length L give
  // (L - k + 1) / (L + 1) (0.58 at k = 63), so the first batch's exact count is read back once (one early wait for its P1)
  // to size the others.
  if((t->item128 || t->item256) && t->items_per_byte <= 0) {
    const uint32_t nb = 1u << t->pg.b1;
    const PendingBatch& pb = t->pending.front();
    if(pb.gran_cap && pb.input_bytes >= (1u << 20)) {
      std::vector<uint64_t> tot(nb);
      HIP_TRY(hipMemcpyAsync(tot.data(), pb.tot, nb * sizeof(uint64_t), hipMemcpyDeviceToHost, t->stream));
      HIP_TRY(hipStreamSynchronize(t->stream));
      uint64_t n = 0; for(uint64_t v : tot) n += v;
      t->items_per_byte = std::max(0.01, (double)n / (double)pb.input_bytes);
    }
  }
  if(!t->wide && t->bcache_state == 0 && t->dt.bloom.data) return bloom_cache_decide(t);
  return JFGPU_OK;
}

// The kernels of a planned P1 batch (ProfScope 4 is open around them).
int run_p1(jfgpu_table* t, const P1Plan& p, const uint8_t* base, int64_t lo, int64_t hi, const PendingBatch& b, unsigned int* gcur) {
  const dim3 grid(p.grid), block(kPBlock);
  const uint32_t nb = 1u << t->pg.b1, gcap = p.gran_cap;
  bool found = false;
  int lrc = JFGPU_OK;               // what a launch with dynamic LDS returned (launch_lds)
  ++(p.kind == kP1Ring ? t->n_p1_ring : t->n_p1_other);
  if(p.kind == kP1NWordGranule) {
    if(t->tun.flush_trace) fprintf(stderr, "[jfgpu flush] P1: p1_nword_granule_kernel, %u buckets, regions of %u items\n", nb, gcap);
    found = pick<Inst<1>, Inst<0>>(p.targs, [&](auto I) {
      lrc = launch_lds(p1_nword_granule_kernel<decltype(I)::v[0] != 0>, grid, block, p.lds, t->stream, t->nt, t->pg, base, lo, hi, gcap, gcur, b.tot, (u256*)b.items);
    });
  } else if(p.kind == kP1WideGranule) {
    found = pick<Inst<1, 0, 1>, Inst<0, 0, 1>, Inst<1, 1, 0>, Inst<1, 0, 0>, Inst<0, 1, 0>, Inst<0, 0, 0>>(p.targs, [&](auto I) {
      constexpr auto& A = decltype(I)::v;
      lrc = launch_lds(p1_wide_granule_kernel<A[0] != 0, A[1] != 0, A[2] != 0>, grid, block, p.lds, t->stream, t->wt, t->pg, base, lo, hi, gcap, gcur, b.tot, (u128*)b.items);
    });
  } else if(p.kind == kP1Granule64) {
    found = pick<Inst<1, 1, 0>, Inst<0, 1, 0>, Inst<1, 0, kHashXS>, Inst<0, 0, kHashXS>, Inst<1, 0, 0>, Inst<0, 0, 8>, Inst<0, 0, 7>, Inst<0, 0, 0>>(p.targs, [&](auto I) {
      constexpr auto& A = decltype(I)::v;
      lrc = launch_lds(p1_granule64_kernel<A[0] != 0, A[1] != 0, A[2]>, grid, block, p.lds, t->stream, t->dt, t->pg, base, lo, hi, gcap, gcur, b.tot, (uint64_t*)b.items);
    });
  } else if(p.kind == kP1KeysGranule) {
    found = pick<Inst<1, 0>, Inst<0, 6>, Inst<0, 7>, Inst<0, 8>, Inst<0, 0>>(p.targs, [&](auto I) {
      constexpr auto& A = decltype(I)::v;
      lrc = launch_lds(p1_keys_granule_kernel<A[0] != 0, A[1]>, grid, block, p.lds, t->stream, t->dt, t->pg, (const uint64_t*)base, hi, gcap, gcur, b.tot, (uint32_t*)b.items);
    });
  } else if(p.kind == kP1Ring) {
    // what cannot be stored in a region (p1_stragglers_kernel) reads the table's descriptor from device memory
    { int rc = refresh_d_dt(t); if(rc) return rc; }
    { int rc = ensure_strag(t); if(rc) return rc; }
    const OneWordDirect od{t->d_dt, t->pg.b2, (int)t->returning};
    unsigned long long* ctr = (unsigned long long*)&t->dt.counters[CTR_DIRECT];
    found = pick<Inst<0, kHashXS, 1>, Inst<0, kHashXS, 0>, Inst<0, kHashXSLow, 2>, Inst<0, 6, 1>, Inst<0, 6, 0>, Inst<1, 0, 2>, Inst<0, 0, 2>>(p.targs, [&](auto I) {
      constexpr auto& A = decltype(I)::v;
      lrc = launch_lds(p1_ring_kernel<uint32_t, A[0] != 0, A[1], A[2]>, grid, block, p.lds, t->stream, t->dt, od, t->pg, base, lo, hi, gcap, gcur, b.tot, (uint32_t*)b.items,
                       t->d_strag.get(), t->d_strag_n.get());
    });
    if(lrc) return lrc;
    hipLaunchKernelGGL((p1_stragglers_kernel<uint32_t, OneWordDirect>), dim3(t->n_cu), dim3(256), 0, t->stream, od, ctr, (const uint64_t*)t->d_strag, (const uint32_t*)t->d_strag_n,
                       (uint32_t)t->n_cu, gcap, gcur, b.tot, (uint32_t*)b.items);
  } else {
    // the exact scheme: count, scan, scatter
    if(!(t->item32 ? launch_p1<uint32_t>(t, p.count_targs, base, lo, hi, b.off, b.items) : launch_p1<uint64_t>(t, p.count_targs, base, lo, hi, b.off, b.items)))
      return no_kernel("p1_kernel (count)");
    hipLaunchKernelGGL(scan_matrix_kernel, dim3(1), dim3(1024), 0, t->stream, t->d_M1, (uint32_t)t->g1, nb, (const uint64_t*)nullptr, b.off, 0u);
    if(p.kind == kP1ExactSorted)
      found = pick<Inst<0, 0, 6>, Inst<0, 0, 7>, Inst<0, 0, 8>, Inst<1, 1, 0>, Inst<1, 0, 0>, Inst<0, 1, 0>, Inst<0, 0, 0>>(p.targs, [&](auto I) {
        constexpr auto& A = decltype(I)::v;
        lrc = launch_lds(p1_scatter_sorted_kernel<A[0] != 0, A[1] != 0, A[2]>, grid, block, p.lds, t->stream, t->dt, t->pg, base, lo, hi, (const uint32_t*)t->d_M1, (const uint64_t*)b.off, (uint32_t*)b.items);
      });
    else if(p.kind == kP1ExactKeysSorted)
      found = pick<Inst<6>, Inst<7>, Inst<8>, Inst<0>>(p.targs, [&](auto I) {
        lrc = launch_lds(p1_keys_scatter_sorted_kernel<decltype(I)::v[0]>, grid, block, p.lds, t->stream, t->dt, t->pg, (const uint64_t*)base, hi, (const uint32_t*)t->d_M1, (const uint64_t*)b.off, (uint32_t*)b.items);
      });
    else found = launch_p1<uint64_t>(t, p.targs, base, lo, hi, b.off, b.items);
  }
  if(!found) return no_kernel("P1");
  if(lrc) return lrc;
  if(gcap) hipLaunchKernelGGL(granule_finish_kernel, dim3((nb + 255) / 256), dim3(256), 0, t->stream, gcur, gcap, nb, b.off);
  return JFGPU_OK;
}

// One batch (contract buffer or key array, on the device) through P1 into a pending batch.
int part_ingest(jfgpu_table* t, const uint8_t* base, int64_t lo, int64_t hi, bool from_keys, uint64_t max_items) {
  if(!max_items) return JFGPU_OK;
  const uint32_t nb = 1u << t->pg.b1;
  if(!t->d_M1) {
    t->g1 = 2 * t->n_cu;   // two 1024-thread blocks per CU: one stages while the other computes
    const int rc = t->d_M1.alloc((size_t)t->g1 * kMaxBuckets); if(rc) return rc;
  }
  auto plan = [&] {
    PendingSum pend{t->pending.size(), 0};
    for(const PendingBatch& pb : t->pending) pend.input_bytes += pb.input_bytes;
    return p1_plan(part_facts(t), from_keys, max_items, lo, hi, pend);
  };
  // (a full list of batches goes before the estimates are read: the flush refreshes them itself)
  if(plan().flush == kFlushSegments) { int rc = part_flush(t); if(rc) return rc; }
  { int rc = refresh_estimates(t, from_keys); if(rc) return rc; }
  const P1Plan p = plan();
  if(p.refuse) return -1;
  if(p.flush) { int rc = part_flush(t); if(rc) return rc; }     // the arena is empty again; the plan's sizes stand
  { int rc = ws_grow(t, p.arena); if(rc) return rc; }           // rc < 0: no memory -> caller goes direct
  PendingBatch b{nullptr, nullptr, max_items};
  b.input_bytes = from_keys ? 0 : (uint64_t)(hi - lo);
  b.bound = t->cur_bound;
  b.gran_cap = p.gran_cap;
  b.items = ws_alloc(t, p.bytes);
  b.off = (uint64_t*)ws_alloc(t, (2 * nb + 1) * sizeof(uint64_t));
  // one pass: reservations of kGran items inside fixed bucket regions -- gcur[2 nb] (u32) then tot[nb] (u64)
  unsigned int* gcur = p.gran_cap ? (unsigned int*)ws_alloc(t, nb * 16) : nullptr;
  if(!b.items || !b.off || (p.gran_cap && !gcur)) return fail(JFGPU_E_ALLOC, "partition workspace exhausted");
  if(gcur) {
    b.tot = (unsigned long long*)(gcur + 2 * nb);
    HIP_TRY(hipMemsetAsync(gcur, 0, nb * 16, t->stream));
  }
  {
    ProfScope ps(t, 4, (uint64_t)(from_keys ? hi : hi - lo));
    const int rc = run_p1(t, p, base, lo, hi, b, gcur); if(rc) return rc;
  }
  hipError_t e = hipGetLastError();
  t->pending.push_back(b);
  t->pending_bytes += p.bytes;
  if(e != hipSuccess) return fail(JFGPU_E_HIP, hipGetErrorString(e));
  return JFGPU_OK;
}

// ---- a flush, first part: what is pending, bucket by bucket ------------------------------------------------------------
// offs: for every pending batch the running sum of its nb1 bucket sizes (nb1 + 1 entries); bucket_tot: items per P1 bucket
// over all batches.  One small copy per batch, which also drains the stream.  Side effects: the capacity accounting is
// corrected from "one k-mer per input byte" to the exact counts, and items_per_byte (what sizes the next batches' regions)
// is refreshed.
struct FlushSizes { std::vector<uint64_t> offs, bucket_tot; uint64_t total = 0; };
int flush_sizes(jfgpu_table* t, FlushSizes& fs) {
  const uint32_t nb1 = 1u << t->pg.b1;
  const size_t nbatch = t->pending.size();
  // bucket sizes of every pending batch (one small D2H; also drains the stream)
  // (granule batches: the exact per-bucket counts, stored as a running sum so both kinds read alike)
  std::vector<uint64_t>& offs = fs.offs;
  offs.assign(nbatch * (nb1 + 1), 0);
  for(size_t s = 0; s < nbatch; ++s) {
    const PendingBatch& pb = t->pending[s];
    if(pb.gran_cap) HIP_TRY(hipMemcpyAsync(&offs[s * (nb1 + 1) + 1], pb.tot, nb1 * sizeof(uint64_t), hipMemcpyDeviceToHost, t->stream));
    else HIP_TRY(hipMemcpyAsync(&offs[s * (nb1 + 1)], pb.off, (nb1 + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, t->stream));
  }
  uint64_t ctr[CTR_COUNT];
  HIP_TRY(hipMemcpyAsync(ctr, t->dt.counters, sizeof(ctr), hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  for(size_t s = 0; s < nbatch; ++s)
    if(t->pending[s].gran_cap) {
      uint64_t* o = &offs[s * (nb1 + 1)];
      o[0] = 0;
      for(uint32_t j = 0; j < nb1; ++j) o[j + 1] += o[j];
    }
  std::vector<uint64_t>& bucket_tot = fs.bucket_tot;
  bucket_tot.assign(nb1, 0);
  uint64_t total = 0, max_bucket = 0;
  for(size_t s = 0; s < nbatch; ++s)
    for(uint32_t j = 0; j < nb1; ++j) bucket_tot[j] += offs[s * (nb1 + 1) + j + 1] - offs[s * (nb1 + 1) + j];
  for(uint32_t j = 0; j < nb1; ++j) { total += bucket_tot[j]; max_bucket = std::max(max_bucket, bucket_tot[j]); }
  if(max_bucket > 0xF0000000ull) return fail(JFGPU_E_UNSUPPORTED, "more than 2^32 pending k-mers in one partition bucket: sync more often");
  {   // capacity accounting (ensure_capacity): these batches were charged one k-mer per input byte, now their exact item
      // counts are known -- plus whatever went straight to the table since the last look
    uint64_t charged = 0, exact = 0;
    for(size_t s = 0; s < nbatch; ++s) if(t->pending[s].bound) { charged += t->pending[s].bound; exact += offs[s * (nb1 + 1) + nb1]; }
    const uint64_t dd = ctr[CTR_DIRECT] >= t->direct_seen ? ctr[CTR_DIRECT] - t->direct_seen : 0;
    t->direct_seen = ctr[CTR_DIRECT];
    if(charged && exact + dd < charged) t->fed_since -= std::min(t->fed_since, charged - (exact + dd));
  }
  {   // items per input byte of what is being flushed (sequence batches only): sizes the next batches' bucket regions
    uint64_t in_bytes = 0, in_items = 0;
    for(size_t s = 0; s < nbatch; ++s)
      if(t->pending[s].input_bytes) { in_bytes += t->pending[s].input_bytes; in_items += offs[s * (nb1 + 1) + nb1]; }
    if(in_bytes >= (1u << 20)) t->items_per_byte = (double)in_items / (double)in_bytes;
  }
  fs.total = total;
  if(t->bcache_state == 0) {       // count --bc, cache of admitted k-mers still undecided: this flush's batches tell (bloom_cache_decide's rule)
    const uint64_t windows = ctr[CTR_MERS] >= t->mers_seen ? ctr[CTR_MERS] - t->mers_seen : 0;
    t->mers_seen = ctr[CTR_MERS];
    if(!t->wide && t->dt.bloom.data && windows >= (1u << 20)) {
      if(total * 100 < windows * 15) t->bcache_state = -1;
      else { const int rc = bloom_cache_enable(t); if(rc) return rc; }
    }
  }
  return JFGPU_OK;
}

// ---- the tile insert of one-word keys (kernels_tile.hip.hpp) --------------------------------------------------------
// One instantiation of tile_rank_insert_kernel over tiles [tile0, tile0 + TPB * ntile): HV the HEAVY variant, SM the plain
// one with its two sample counters on.
// HL: the hole-aware instantiation.  The one for hole-free regions (SegList::dense) exists where such regions do: 4-byte
// items into pairs of tiles, the plain kernel (HEAVY keeps the hole-aware code on both kinds of input).
template <typename ITEM, typename SLOT, int TPB, bool HV, bool SM, bool HL>
int launch_tile_rank_inst(jfgpu_table* t, const SegList& S, uint64_t tile0, uint32_t ntile, hipStream_t ts) {
  const size_t lds = tile_rank_lds(sizeof(SLOT), t->g.tile_bits, TPB);
  const dim3 grid((unsigned)std::min<uint64_t>(ntile, (uint64_t)t->n_cu * 16)), block(kTileBlock);
  int rc = JFGPU_OK;
  with_flags(t->returning, [&](auto RT) {      // a tile is read only if its dirty byte is set (clean after jfgpu_clear)
    rc = launch_lds(tile_rank_insert_kernel<ITEM, decltype(RT)::value, SLOT, TPB, kTileBlock, HV, SM, HL>, grid, block, lds, ts, t->dt, S, tile0, ntile);
  });
  return rc;
}
template <typename ITEM, typename SLOT, int TPB, bool HV, bool SM>
int launch_tile_rank_variant(jfgpu_table* t, const SegList& S, uint64_t tile0, uint32_t ntile, hipStream_t ts) {
  if constexpr(sizeof(ITEM) == 4 && TPB == 2 && !HV) {
    if(S.n == 1 && S.sh[0] == 1 && S.dense[0]) { ++t->n_tile_dense; return launch_tile_rank_inst<ITEM, SLOT, TPB, HV, SM, false>(t, S, tile0, ntile, ts); }
  }
  return launch_tile_rank_inst<ITEM, SLOT, TPB, HV, SM, true>(t, S, tile0, ntile, ts);
}
// Which instantiation (plain, or HEAVY for high-coverage input) is decided from the flush itself: the first `sample` units
// of a large launch (a 64th: tile_sample_units) go through the plain kernel with its counters on, the host reads them (one
// wait inside the flush) and the rest follows in the instantiation they call for.  JFGPU_TILE_ADAPT=0: always plain; 2: always
// HEAVY (tests).
template <typename ITEM, typename SLOT, int TPB>
int launch_tile_rank(jfgpu_table* t, const SegList& S, uint64_t tile0, uint32_t ntile, uint32_t sample, hipStream_t ts) {
  bool heavy = t->tun.tile_adapt == 2;
  if(sample) {
    (void)hipMemsetAsync(&t->dt.counters[CTR_T_ITEMS], 0, 2 * sizeof(uint64_t), ts);
    { const int rc = launch_tile_rank_variant<ITEM, SLOT, TPB, false, true>(t, S, tile0, sample, ts); if(rc) return rc; }
    uint64_t smp[2] = {0, 0};                              // items placed, items past rank 3
    if(hipMemcpyAsync(smp, &t->dt.counters[CTR_T_ITEMS], sizeof smp, hipMemcpyDeviceToHost, ts) == hipSuccess && hipStreamSynchronize(ts) == hipSuccess)
      heavy = smp[1] * 4 > smp[0];
  }
  SegList Sr = S; Sr.off[0] = S.off[0] + ((size_t)sample << S.sh[0]);
  if(heavy) ++t->flushes_heavy; else ++t->flushes_plain;
  if(heavy) return launch_tile_rank_variant<ITEM, SLOT, TPB, true, false>(t, Sr, tile0 + (uint64_t)TPB * sample, ntile - sample, ts);
  return launch_tile_rank_variant<ITEM, SLOT, TPB, false, false>(t, Sr, tile0 + (uint64_t)TPB * sample, ntile - sample, ts);
}

// the tile insert of one item array (or of the pending batches themselves), on stream `ts`
template <typename ITEM>
int launch_tile_kernel(jfgpu_table* t, const SegList& S, uint64_t tile0, uint32_t ntile, uint32_t sample, hipStream_t ts, bool pair) {
  if constexpr(sizeof(ITEM) == 32) {
    // keys of three and four words: 256-bit items, 256-bit slots; 64 KiB of LDS: two blocks per CU
    const size_t tile_lds = (size_t)32 << t->g.tile_bits;
    const dim3 block(kNTileBlock), grid((unsigned)std::min<uint64_t>(ntile, (uint64_t)t->n_cu * 8));
    ++t->n_tile_nword;
    if(t->tun.flush_trace) fprintf(stderr, "[jfgpu flush] T: tile_insert_nword_kernel, %u tiles from %llu, %u segment(s)\n", ntile, (unsigned long long)tile0, S.n);
    int rc = JFGPU_OK;
    with_flags(t->returning, [&](auto RT) { rc = launch_lds(tile_insert_nword_kernel<decltype(RT)::value>, grid, block, tile_lds, ts, t->nt, S, tile0, ntile); });
    return rc;
  } else if constexpr(sizeof(ITEM) == 16) {
    // two-word keys: 128-bit items, 128-bit slots; 128 KiB of LDS: one block per CU
    const size_t tile_lds = (size_t)16 << t->g.tile_bits;
    const bool pipe = S.n == 1 && t->tun.wide_pipe;        // one item array (a flush's P2 output): the pipelined kernel
    const dim3 block(kPBlock), grid((unsigned)std::min<uint64_t>(ntile, (uint64_t)t->n_cu * (pipe ? 1 : 4)));
    int rc = JFGPU_OK;
    with_flags(t->returning, [&](auto RT) {
      if(pipe) rc = launch_lds(tile_insert_wide_pipe_kernel<decltype(RT)::value>, grid, block, tile_lds, ts, t->wt, S, tile0, ntile);
      else     rc = launch_lds(tile_insert_wide_kernel<decltype(RT)::value>, grid, block, tile_lds, ts, t->wt, S, tile0, ntile);
    });
    return rc;
  } else {
    // one-word keys: placement by rank inside buckets of four (kernels_tile.hip.hpp); two workgroups per CU
    if(t->g.slot32) return pair ? launch_tile_rank<ITEM, unsigned int, 2>(t, S, tile0, ntile, sample, ts) : launch_tile_rank<ITEM, unsigned int, 1>(t, S, tile0, ntile, sample, ts);
    return launch_tile_rank<ITEM, unsigned long long, 1>(t, S, tile0, ntile, sample, ts);
  }
}

// kRouteDirect: global atomics straight from the pending items, batch by batch
template <typename ITEM>
void run_items_direct(jfgpu_table* t, const FlushSizes& fs) {
  const uint32_t nb1 = 1u << t->pg.b1;
  for(size_t s = 0; s < t->pending.size(); ++s) {
    const PendingBatch& pb = t->pending[s];
    const uint64_t n = fs.offs[s * (nb1 + 1) + nb1], gc = pb.gran_cap;
    if(!n) continue;
    ProfScope ps(t, 7, n);
    const uint64_t span = gc ? (uint64_t)nb1 * gc : n;
    const dim3 grid((unsigned)grid_for(t, (span + kBlock - 1) / kBlock)), block(kBlock);
    with_flags(t->returning, [&](auto RT) {
      if constexpr(sizeof(ITEM) == 32) hipLaunchKernelGGL(items_direct_nword_kernel<decltype(RT)::value>, grid, block, 0, t->stream, t->nt, t->pg, (const u256*)pb.items, (const uint64_t*)pb.off, gc);
      else if constexpr(sizeof(ITEM) == 16) hipLaunchKernelGGL(items_direct_wide_kernel<decltype(RT)::value>, grid, block, 0, t->stream, t->wt, t->pg, (const u128*)pb.items, (const uint64_t*)pb.off, gc);
      else hipLaunchKernelGGL((items_direct_kernel<ITEM, decltype(RT)::value>), grid, block, 0, t->stream, t->dt, t->pg, (const ITEM*)pb.items, (const uint64_t*)pb.off, gc);
    });
  }
}

// kRouteSingleLevel: the P1 buckets are the tiles; keys of two and more words take all batches in one pass, one-word keys one pass a batch
template <typename ITEM>
int run_single_level(jfgpu_table* t, const PartFacts& f, const FlushSizes& fs, const SegList& S1) {
  const uint32_t nb1 = 1u << t->pg.b1;
  auto launch_tiles = [&](const SegList& S, uint64_t units) {
    ProfScope ps(t, 6, units);
    return launch_tile_kernel<ITEM>(t, S, 0, nb1, tile_sample_units(f, nb1, S.n), t->stream, false);
  };
  if constexpr(sizeof(ITEM) >= 16) return launch_tiles(S1, fs.total);
  else for(size_t s = 0; s < S1.n; ++s) {
    const uint64_t n = fs.offs[s * (nb1 + 1) + nb1];
    if(!n) continue;
    SegList Sb; memset(&Sb, 0, sizeof Sb);
    Sb.n = 1; Sb.items[0] = S1.items[s]; Sb.off[0] = S1.off[s]; Sb.sh[0] = S1.sh[s];
    const int rc = launch_tiles(Sb, n); if(rc) return rc;
  }
  return JFGPU_OK;
}

// The three blocks of a two-level flush (FlushPlan::block_*): from the arena where the plan put them, or -- one_off -- held
// by `own` until the flush returns, whichever way (hipFree waits for the kernels still reading them).  *struck: the
// single pass's one-off blocks could not be had, which is no error: the caller plans again without them.
int take_blocks(jfgpu_table* t, const FlushPlan& p, DevBuf<uint8_t> (&own)[3], void* (&blk)[3], bool* struck) {
  if(!p.one_off) {
    for(int i = 0; i < 3; ++i) {
      blk[i] = ws_alloc(t, p.block_bytes[i]);
      if(blk[i] != t->ws + p.block_at[i]) return fail(JFGPU_E_ALLOC, "partition plan and arena disagree");
    }
  } else if(p.cap2) {
    if(!(own[0].try_alloc(p.block_bytes[0]) && own[1].try_alloc(p.block_bytes[1]) && own[2].try_alloc(p.block_bytes[2]))) {
      for(auto& o : own) (void)o.reset();
      *struck = true;
      return JFGPU_OK;
    }
  } else {
    if(p.no_memory) return fail(JFGPU_E_ALLOC, "hipMalloc partition temporaries");
    { const int rc = own[2].alloc(p.block_bytes[2]); if(rc) return rc; }
    if(!own[0].try_alloc(p.block_bytes[0]) || !own[1].try_alloc(p.block_bytes[1])) return fail(JFGPU_E_ALLOC, "hipMalloc partition offsets");
  }
  if(p.one_off) for(int i = 0; i < 3; ++i) blk[i] = own[i].get();
  return JFGPU_OK;
}

// P2 of one bucket group, by the plan's kind, and the finish kernel; *S2: what the tile insert reads.
template <typename ITEM>
int run_p2(jfgpu_table* t, const FlushPlan& p, const GroupPlan& q, const SegList& S1, void* const (&blk)[3], SegList* S2) {
  const dim3 grid(q.grid_x, q.grid_y), block(kPBlock);
  memset(S2, 0, sizeof *S2);
  S2->n = 1;
  if(q.p2 == kP2Exact) {
    uint64_t *d_goff = (uint64_t*)blk[0], *d_base = (uint64_t*)blk[1]; ITEM* tmp = (ITEM*)blk[2];
    PartGeom pg2 = t->pg; pg2.b2 = p.b2e;
    ++t->n_p2_exact;
    hipLaunchKernelGGL((p2_kernel<ITEM, false>), grid, block, 0, t->stream, pg2, p.p2_tag_bits, S1, t->d_M2, (const uint64_t*)d_goff, tmp, q.b0);
    hipLaunchKernelGGL(scan_matrix_kernel, dim3(q.nbk), dim3(1024), 0, t->stream, t->d_M2, kG2Exact, 1u << p.b2e, (const uint64_t*)d_base, d_goff, q.b0);
    int rc = JFGPU_OK;
    auto scatter = [&](auto I) {
      rc = launch_lds(p2_scatter_sorted_kernel<ITEM, decltype(I)::v[0]>, grid, block, q.lds, t->stream, pg2, p.p2_tag_bits, S1, (const uint32_t*)t->d_M2, (const uint64_t*)d_goff, tmp, q.b0);
    };
    bool found;
    if constexpr(sizeof(ITEM) == 4) found = pick<Inst<kP2PairPer>, Inst<16>>(q.p2_targs, scatter);
    else found = pick<Inst<sizeof(ITEM) == 8 ? 14 : sizeof(ITEM) == 16 ? 7 : kP2NWordPer>>(q.p2_targs, scatter);
    if(!found) return no_kernel("p2_scatter_sorted_kernel");
    if(rc) return rc;
    S2->items[0] = tmp; S2->off[0] = d_goff + q.d0;
    return JFGPU_OK;
  }
  // single pass: destination d of the whole table sits at d * cap2 of a buffer that only holds this group's (shifted base)
  unsigned int* d_gcur2 = (unsigned int*)blk[0]; uint64_t* d_off2 = (uint64_t*)blk[1];
  ITEM* out_v = (ITEM*)blk[2] - (p.share ? (int64_t)q.d0 * (int64_t)p.cap2 : 0);
  if constexpr(sizeof(ITEM) == 32) return no_kernel("single-pass P2 of 32-byte items");
  else {
  if(q.p2 == kP2Sort) {
    constexpr int per = sizeof(ITEM) == 4 ? kP2PairPer : sizeof(ITEM) == 8 ? kP2MidPer : kP2WidePer;
    ++t->n_p2_sort;
    int rc = JFGPU_OK;
    with_flags(t->returning, [&](auto RT) {
      constexpr bool rt = decltype(RT)::value;
      const auto direct = [&] {      // what does not fit a region goes straight to the table
        if constexpr(sizeof(ITEM) == 16) return WideDirect<rt>{t->wt, t->pg};
        else return TableDirect<rt>{t->d_dt, t->pg, (unsigned long long*)&t->dt.counters[CTR_DIRECT]};
      }();
      rc = launch_lds(p2_granule_kernel<ITEM, std::remove_const_t<decltype(direct)>, per>, grid, block, q.lds, t->stream, direct, p.b2e, p.p2_tag_bits, S1, p.cap2, d_gcur2, d_gcur2 + p.n_dest, out_v, q.b0,
                      (unsigned long long*)nullptr, 0xFFFFFFFFu);      // (no totals, every bucket: the kernel's defaults, which a function pointer does not carry)
    });
    if(rc) return rc;
  } else if constexpr(sizeof(ITEM) == 4) {
    const int rc = launch_p2_rings(t, p, q, S1, d_gcur2, out_v); if(rc) return rc;
  } else return no_kernel("ring P2 of items wider than 4 bytes");
  // (granule_finish_kernel reads gcur[nb + j] as destination j's overflow note: the two halves of d_gcur2)
  if(p.n_groups == 1) hipLaunchKernelGGL(granule_finish_kernel, dim3(1024), dim3(256), 0, t->stream, d_gcur2, p.cap2, (uint32_t)p.n_dest, d_off2);
  else hipLaunchKernelGGL(granule_finish_range_kernel, dim3(256), dim3(256), 0, t->stream, d_gcur2, p.cap2, (uint32_t)p.n_dest, d_off2, (uint32_t)q.d0, (uint32_t)q.nd);
  // offsets from the group's first destination, items absolute
  S2->items[0] = out_v; S2->off[0] = d_off2 + 2 * q.d0; S2->sh[0] = 1; S2->dense[0] = q.dense;
  return JFGPU_OK;
  }
}

// The tile insert of group g behind its P2, with the profile spans that go with the plan: groups sharing a buffer run P2
// and the tile insert in turn on one stream and every group's two stages are timed on their own (`ga`: recorded before the
// group's P2); otherwise one P2 span and one tile span over the whole flush (`whole`: p2a, p2b, ta, tb), and with two streams
// the tile insert waits for the group's P2 on the second one.
template <typename ITEM>
int tile_stage(jfgpu_table* t, const FlushPlan& p, const GroupPlan& q, uint32_t g, const SegList& S2, hipEvent_t ga, hipEvent_t (&whole)[4]) {
  hipStream_t ts = t->stream;
  const bool prof = t->prof_on, last = g + 1 == p.n_groups;
  if(p.share) {
    hipEvent_t gb = nullptr, gc = nullptr, gd = nullptr;
    if(prof) {
      gb = get_event(t); gc = get_event(t); gd = get_event(t);
      hipEventRecord(gb, ts); hipEventRecord(gc, ts);
      t->prof_pending.push_back({ga, gb, 5, q.items});
    }
    { const int rc = launch_tile_kernel<ITEM>(t, S2, q.tile0, q.ntile, q.sample, ts, p.pair); if(rc) return rc; }
    if(prof) { hipEventRecord(gd, ts); t->prof_pending.push_back({gc, gd, 6, q.items}); }
    return JFGPU_OK;
  }
  if(prof && last) hipEventRecord(whole[1], t->stream);
  if(p.two_streams) {
    HIP_TRY(hipEventRecord(t->flush_ev[g & 1], t->stream));
    HIP_TRY(hipStreamWaitEvent(t->stream2, t->flush_ev[g & 1], 0));
    ts = t->stream2;
  }
  if(prof && g == 0) hipEventRecord(whole[2], ts);
  { const int rc = launch_tile_kernel<ITEM>(t, S2, q.tile0, q.ntile, q.sample, ts, p.pair); if(rc) return rc; }
  if(prof && last) hipEventRecord(whole[3], ts);
  return JFGPU_OK;
}

// kRouteTwoLevel: every P1 bucket through P2, then every tile, group by group
template <typename ITEM>
int run_two_level(jfgpu_table* t, const PartFacts& f, FlushPlan p, const FlushSizes& fs, const SegList& S1, bool all_granule) {
  const uint32_t nb1 = 1u << t->pg.b1;
  const uint64_t* bucket_tot = fs.bucket_tot.data();
  if(!t->d_M2) { const int rc = t->d_M2.alloc((size_t)nb1 * kG2Exact << t->pg.b2); if(rc) return rc; }
  DevBuf<uint8_t> own[3];
  void* blk[3] = {nullptr, nullptr, nullptr};
  for(FlushAllow allow;;) {
    bool struck = false;
    const int rc = take_blocks(t, p, own, blk, &struck); if(rc) return rc;
    if(!struck) break;
    allow.single_one_off = false;
    p = flush_plan(f, fs.total, bucket_tot, S1.n, all_granule, allow);
  }
  if(t->tun.flush_trace) {
    fprintf(stderr, "[flush] %llu items in %zu batches, %llu tiles, pairs %d, single-pass P2 regions of %u items (0: exact P2) in %u group(s)\n",
            (unsigned long long)fs.total, (size_t)S1.n, (unsigned long long)f.n_tiles, (int)p.pair, p.cap2, p.cap2 ? p.n_groups : 1);
    if(!p.cap2 && p.share) fprintf(stderr, "[flush] P2 + tile insert in %u groups sharing an output buffer of %llu items\n", p.n_groups, (unsigned long long)p.tmp_items);
  }
  if(p.cap2) HIP_TRY(hipMemsetAsync(blk[0], 0, p.block_bytes[0], t->stream));
  else {
    std::vector<uint64_t> base(nb1);                     // where a bucket's tiles start in tmp (groups sharing tmp: from 0 again)
    uint64_t run = 0;
    for(uint32_t j = 0; j < nb1; ++j) { if(p.share && j % (nb1 / p.n_groups) == 0) run = 0; base[j] = run; run += bucket_tot[j]; }
    HIP_TRY(hipMemcpyAsync(blk[1], base.data(), nb1 * sizeof(uint64_t), hipMemcpyHostToDevice, t->stream));
  }
  if(p.two_streams && !t->stream2) {
    int rc;
    if((rc = t->stream2.create()) || (rc = t->flush_ev[0].create(hipEventDisableTiming)) || (rc = t->flush_ev[1].create(hipEventDisableTiming)) ||
       (rc = t->flush_done.create(hipEventDisableTiming))) return rc;
  }
  hipEvent_t whole[4] = {nullptr, nullptr, nullptr, nullptr};      // p2a, p2b, ta, tb
  if(t->prof_on && !p.share) { for(hipEvent_t& e : whole) e = get_event(t); hipEventRecord(whole[0], t->stream); }
  for(uint32_t g = 0; g < p.n_groups; ++g) {
    const GroupPlan q = group_plan(f, p, g, bucket_tot, all_granule);
    hipEvent_t ga = nullptr;
    if(t->prof_on && p.share) { ga = get_event(t); hipEventRecord(ga, t->stream); }
    SegList S2;
    { const int rc = run_p2<ITEM>(t, p, q, S1, blk, &S2); if(rc) return rc; }
    { const int rc = tile_stage<ITEM>(t, p, q, g, S2, ga, whole); if(rc) return rc; }
  }
  if(t->prof_on && !p.share) {
    t->prof_pending.push_back({whole[0], whole[1], 5, fs.total});
    t->prof_pending.push_back({whole[2], whole[3], 6, fs.total});
  }
  if(p.two_streams) {        // the table's stream continues only after the last tiles are in
    HIP_TRY(hipEventRecord(t->flush_done, t->stream2));
    HIP_TRY(hipStreamWaitEvent(t->stream, t->flush_done, 0));
  }
  const hipError_t e = hipStreamSynchronize(t->stream);          // (before `own` goes)
  if(e != hipSuccess) return fail(JFGPU_E_HIP, hipGetErrorString(e));
  return JFGPU_OK;
}

template <typename ITEM>
int part_flush_t(jfgpu_table* t) {
  FlushSizes fs;
  { const int rc = flush_sizes(t, fs); if(rc) return rc; }
  if constexpr(sizeof(ITEM) < 16) { int rc = refresh_d_dt(t); if(rc) return rc; }
  const PartFacts f = part_facts(t);
  SegList S1; memset(&S1, 0, sizeof S1);
  S1.n = (uint32_t)t->pending.size();
  bool all_granule = true;
  for(size_t s = 0; s < S1.n; ++s) {
    const PendingBatch& pb = t->pending[s];
    S1.items[s] = pb.items; S1.off[s] = pb.off; S1.sh[s] = pb.gran_cap ? 1 : 0;
    all_granule = all_granule && pb.gran_cap != 0;
  }
  const FlushPlan p = flush_plan(f, fs.total, fs.bucket_tot.data(), S1.n, all_granule, FlushAllow{});
  switch(p.route) {
  case kRouteNothing: break;
  case kRouteDirect: run_items_direct<ITEM>(t, fs); break;
  case kRouteSingleLevel: { const int rc = run_single_level<ITEM>(t, f, fs, S1); if(rc) return rc; } break;
  case kRouteTwoLevel: { const int rc = run_two_level<ITEM>(t, f, p, fs, S1, all_granule); if(rc) return rc; }
  }
  hipError_t e = hipGetLastError();
  if(e == hipSuccess) e = hipStreamSynchronize(t->stream);
  t->pending.clear(); t->pending_bytes = 0; t->ws_used = 0;
  if(fs.total) t->pristine = false;
  if(e != hipSuccess) return fail(JFGPU_E_HIP, hipGetErrorString(e));
  return JFGPU_OK;
}

int part_flush(jfgpu_table* t) {
  if(t->pending.empty()) return JFGPU_OK;
  const int rc = t->item256 ? part_flush_t<u256>(t) : t->item128 ? part_flush_t<u128>(t) : t->item32 ? part_flush_t<uint32_t>(t) : part_flush_t<uint64_t>(t);
  if(rc) {      // what was pending is lost with the failed flush: the table no longer holds what it was fed, and says so until
    if(t->stream) hipStreamSynchronize(t->stream);      // it is cleared (jfgpu_clear), instead of carrying on with k-mers missing
    t->pending.clear(); t->pending_bytes = 0; t->ws_used = 0;
    t->failed = rc; t->failed_msg = jfgpu_last_error();
  }
  return rc;
}

// Replace the charges of the pending batches (one k-mer per input byte) by their exact item counts: one wait for the P1
// kernels already enqueued, no flush.  The batches keep the corrected charge, so the flush's own correction stays neutral.
int refine_pending_charges(jfgpu_table* t) {
  if(t->pending.empty()) return JFGPU_OK;
  const uint32_t nb1 = 1u << t->pg.b1;
  std::vector<size_t> idx;
  for(size_t s = 0; s < t->pending.size(); ++s) if(t->pending[s].bound) idx.push_back(s);
  if(idx.empty()) return JFGPU_OK;
  std::vector<uint64_t> buf(idx.size() * nb1);
  uint64_t ctr[CTR_COUNT];
  for(size_t i = 0; i < idx.size(); ++i) {
    const PendingBatch& pb = t->pending[idx[i]];
    if(pb.gran_cap) HIP_TRY(hipMemcpyAsync(&buf[i * nb1], pb.tot, nb1 * sizeof(uint64_t), hipMemcpyDeviceToHost, t->stream));
    else HIP_TRY(hipMemcpyAsync(&buf[i * nb1], pb.off + nb1, sizeof(uint64_t), hipMemcpyDeviceToHost, t->stream));
  }
  HIP_TRY(hipMemcpyAsync(ctr, t->dt.counters, sizeof(ctr), hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  uint64_t charged = 0, exact = 0;
  for(size_t i = 0; i < idx.size(); ++i) {
    PendingBatch& pb = t->pending[idx[i]];
    uint64_t n = 0;
    if(pb.gran_cap) for(uint32_t j = 0; j < nb1; ++j) n += buf[i * nb1 + j]; else n = buf[i * nb1];
    charged += pb.bound; exact += std::min(n, pb.bound);
    pb.bound = std::max<uint64_t>(std::min(n, pb.bound), 1);
  }
  const uint64_t dd = ctr[CTR_DIRECT] >= t->direct_seen ? ctr[CTR_DIRECT] - t->direct_seen : 0;
  t->direct_seen = ctr[CTR_DIRECT];
  if(exact + dd < charged) t->fed_since -= std::min(t->fed_since, charged - (exact + dd));
  else t->fed_since += (exact + dd) - charged;
  return JFGPU_OK;
}

void part_discard(jfgpu_table* t) {
  if(t->stream) hipStreamSynchronize(t->stream);
  t->pending.clear(); t->pending_bytes = 0; t->ws_used = 0;
}
