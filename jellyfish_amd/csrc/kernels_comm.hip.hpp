// jellyfish_amd/csrc/kernels_comm.hip.hpp -- the small kernels of the multi-GPU exchange (host side: abi_comm.inl):
//   comm_claims_kernel          sender, item path: what every owner is being sent, and the two numbers the host wants back
//   comm_add_claims_kernel      receiver, item path: the senders' claims summed
//   comm_mark_direct_kernel,
//   comm_count_arrived_kernel   receiver, item path: its own count of what arrived, around the receive split
//   reshard_kernel              the shards grow together (comm_grow): what stays, what leaves as (key, count) pairs
//   add_pairs_kernel            (key, count) pairs into a table: comm_grow's arrivals, jfgpu_add_key_vals
//   bloom_merge_kernel          `bc` over several GPUs (comm_bc_merge): two counters' cells added, saturating at 2
// The routing, split and insert kernels of the exchange are the partition path's own (kernels_part.hip.hpp,
// kernels_p1ring.hip.hpp).
#pragma once
#include "kernels.hip.hpp"

namespace jfgpu {

// What every owner is being sent by this rank (its regions' items + its stragglers), written where the exchange takes it
// from (claims[W] of the send buffer), and the two numbers the host wants back (items stored, stragglers): on the device,
// so that the host has nothing to compute between the routing kernel and the exchange.
__global__ __launch_bounds__(1024) void comm_claims_kernel(const unsigned long long* __restrict__ tot, uint32_t nbg, uint32_t nbc, const uint64_t* __restrict__ strag,
                                                            uint32_t S, uint32_t world, uint64_t* __restrict__ claims, uint64_t* __restrict__ summary) {
  __shared__ unsigned long long s_claims[512];
  __shared__ unsigned long long s_stored;
  for(uint32_t p = threadIdx.x; p < world; p += blockDim.x) s_claims[p] = 0;
  if(threadIdx.x == 0) s_stored = 0;
  lds_barrier();
  for(uint32_t j = threadIdx.x; j < nbg; j += blockDim.x) { const unsigned long long v = tot[j]; if(v) { atomicAdd(&s_claims[j / nbc], v); atomicAdd(&s_stored, v); } }
  const uint64_t ns = strag[0];
  const uint64_t nl = ns < S ? ns : S;
  for(uint64_t i = threadIdx.x; i < nl; i += blockDim.x) atomicAdd(&s_claims[(uint32_t)(strag[1 + i] >> 32) / nbc], 1ull);
  lds_barrier();
  for(uint32_t p = threadIdx.x; p < world; p += blockDim.x) claims[p] = s_claims[p];
  if(threadIdx.x == 0) { summary[0] = s_stored; summary[1] = ns; }
}

__global__ void comm_add_claims_kernel(const uint64_t* __restrict__ claims, int n, unsigned long long* __restrict__ total) {
  if(blockIdx.x == 0 && threadIdx.x == 0) { unsigned long long s = 0; for(int i = 0; i < n; ++i) s += claims[i]; *total += s; }
}

// The receiver's own count of what arrived (the claims above are the senders' word): before the split, remember the
// table's direct-insert counter; after it, add what the split stored in its regions (tot[]) and what it inserted directly.
__global__ void comm_mark_direct_kernel(const uint64_t* __restrict__ counters, unsigned long long* __restrict__ arrived) {
  if(blockIdx.x == 0 && threadIdx.x == 0) arrived[1] = counters[CTR_DIRECT];
}
__global__ void comm_count_arrived_kernel(const unsigned long long* __restrict__ tot, uint32_t nb, const uint64_t* __restrict__ counters,
                                          unsigned long long* __restrict__ arrived) {
  unsigned long long s = 0;
  for(uint32_t j = threadIdx.x; j < nb; j += blockDim.x) s += tot[j];
  for(int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if((threadIdx.x & 63) == 0 && s) atomicAdd(&arrived[0], s);
  if(threadIdx.x == 0) atomicAdd(&arrived[0], (unsigned long long)(counters[CTR_DIRECT] - arrived[1]));
}

// ---- the shards of a table grow together -------------------------------------------------------------------------------
// hash_counter::double_size (hash_counter.hpp:200-238) for a table spread over ranks.  The doubled table has a new matrix
// (the next one of the reference's random() stream, the same on every rank), so an entry's owner changes: every rank
// walks its old shard, puts what stays with it into its new shard and sends the rest -- (key, count) pairs, grouped by
// new owner -- through the key path's exchange, twice (keys, then counts, same grouping).  Every key width (KeyOps): a
// pair is kw key words (low first) and a count.
//   pass 0: how many pairs for every owner;  pass 1: the pairs, at the cursors (= offsets), and the local inserts
template <class Table>
__global__ __launch_bounds__(kBlock) void reshard_kernel(Table old, Table neu, int have_ovf, int pass, uint32_t kw, unsigned long long* __restrict__ cursors,
                                                         uint64_t* __restrict__ keys_out, uint64_t* __restrict__ cnts_out) {
  typedef KeyOps<Table> K;
  const TableGeom& g = K::geom(old);
  const uint64_t n = 1ull << g.lsize_l;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    typename K::Slot s;
    if(!K::load(old, i, s)) continue;                    // (a claim that was never completed holds no key)
    const typename K::Key key = K::key(old, s, i & ~g.tile_mask);
    const uint32_t owner = K::owner(neu, neu.fwd_tbl, key);
    if(owner == K::geom(neu).shard_id) { if(pass) K::add_val(neu, neu.fwd_tbl, key, K::count(old, s, i, have_ovf)); }
    else {
      const unsigned long long at = atomicAdd(&cursors[owner], 1ull);
      if(pass) { K::store_key(keys_out + (uint64_t)kw * at, key, kw); cnts_out[at] = K::count(old, s, i, have_ovf); }
    }
  }
}
template <class Table>
__global__ __launch_bounds__(kBlock) void add_pairs_kernel(Table T, const uint64_t* __restrict__ keys, const uint64_t* __restrict__ cnts, uint64_t n, uint32_t kw) {
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    KeyOps<Table>::add_val(T, T.fwd_tbl, KeyOps<Table>::load_key(T, keys, i, kw, false), cnts[i]);      // (keys as they come: made by store_key or by the caller)
}

// ---- `jellyfish bc` over several GPUs: the ranks' counters merged (comm_bc_merge) ------------------------------------------
__device__ __forceinline__ uint32_t bloom_byte_add(uint32_t a, uint32_t b) {     // five base-3 digits a byte, digit-wise min(2, a + b)
  uint32_t r = 0, w = 1;
#pragma unroll
  for(int d = 0; d < 5; ++d) { const uint32_t s = a % 3u + b % 3u; r += (s > 2u ? 2u : s) * w; w *= 3u; a /= 3u; b /= 3u; }
  return r;
}
__global__ __launch_bounds__(kBlock) void bloom_merge_kernel(uint64_t* __restrict__ dst, const uint64_t* __restrict__ src, uint64_t n_words) {
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t a = dst[i], b = src[i];
    if(b == 0) continue;
    uint64_t r = 0;
#pragma unroll
    for(int k = 0; k < 8; ++k) r |= (uint64_t)bloom_byte_add((uint32_t)(a >> (8 * k)) & 0xFFu, (uint32_t)(b >> (8 * k)) & 0xFFu) << (8 * k);
    dst[i] = r;
  }
}

}  // namespace jfgpu
