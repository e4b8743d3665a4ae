// jellyfish_amd/csrc/comm_ipc.inl -- the "ipc" transport of the multi-GPU exchange, included by abi_comm.inl (see its head)
// after the communicator, the item message's layout and the steps the transports share.  One process per rank; the
// messages are copies between the processes' device allocations (hipIpcGetMemHandle / hipIpcOpenMemHandle), the small
// host-level agreements (counts, barriers, allreduce / allgather) live in a POSIX shared-memory block.  The emulated
// build has no such transport: its stubs are at the end.
#if !defined(JFGPU_EMU)
#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>
#include <atomic>
#include <chrono>
#include <thread>

constexpr int kIpcMaxWorld = 16;
struct IpcShared {
  std::atomic<uint32_t> arrived, generation, failed, attached;
  uint64_t coll[kIpcMaxWorld][64];                          // a rank's contribution to the running collective
  struct Pub {
    hipIpcMemHandle_t send[2]; uint64_t send_epoch[2];      // send buffers of both turns (epoch changes when one is re-allocated)
    uint64_t scount[kIpcMaxWorld], soff[kIpcMaxWorld + 1];  // key path: what this rank holds for every owner, and where
  } pub[kIpcMaxWorld];
};

// A rank's attachment to the shared block and what it has mapped of its peers.  Going, it closes the mappings, leaves the
// block and, as the last rank to leave, unlinks it.
struct IpcAttachment {
  IpcShared* shm = nullptr; std::string name;
  struct PeerMap { void* ptr = nullptr; uint64_t epoch = 0; };
  std::vector<PeerMap> peer_send[2];             // peers' send buffers as mapped here, per turn
  std::vector<void*> stale_maps;                 // mappings of send buffers the peers have replaced since (closed with the communicator)
  uint64_t send_epoch[2] = {0, 0}; void* send_exported[2] = {nullptr, nullptr}; size_t send_exported_cap[2] = {0, 0};
  IpcAttachment() = default;
  IpcAttachment(const IpcAttachment&) = delete;
  IpcAttachment& operator=(const IpcAttachment&) = delete;
  ~IpcAttachment() {
    for(int i = 0; i < 2; ++i) for(auto& M : peer_send[i]) if(M.ptr) hipIpcCloseMemHandle(M.ptr);
    for(void* p : stale_maps) hipIpcCloseMemHandle(p);
    if(!shm) return;
    const bool last = shm->attached.fetch_sub(1) == 1;
    munmap(shm, sizeof(IpcShared));
    if(last) shm_unlink(name.c_str());
  }
};

namespace {

int ipc_fail(jfgpu_comm* c, const char* what) {
  if(c->att && c->att->shm) c->att->shm->failed.store(1);
  return fail(JFGPU_E_HIP, std::string("ipc transport: ") + what);
}

// Sense-reversing barrier over the shared block; gives up when a rank reported a failure or nobody moves for 10 minutes.
int ipc_barrier(jfgpu_comm* c) {
  IpcShared* S = c->att->shm;
  const uint32_t gen = S->generation.load();
  if(S->arrived.fetch_add(1) + 1 == (uint32_t)c->world) { S->arrived.store(0); S->generation.fetch_add(1); return JFGPU_OK; }
  const auto t0 = std::chrono::steady_clock::now();
  for(uint64_t spins = 0; S->generation.load() == gen; ++spins) {
    if(S->failed.load()) return fail(JFGPU_E_HIP, "ipc transport: another rank failed");
    if(spins > 2000) std::this_thread::sleep_for(std::chrono::microseconds(50)); else std::this_thread::yield();
    if((spins & 0xFFFF) == 0xFFFF && std::chrono::steady_clock::now() - t0 > std::chrono::minutes(10)) return ipc_fail(c, "barrier timed out");
  }
  return JFGPU_OK;
}

// (Re-)publish this rank's send buffer of turn `cur` if it was re-allocated since.
int ipc_publish_send(jfgpu_comm* c, int cur) {
  jfgpu_comm::Rank& R = c->ranks[0];
  IpcAttachment& A = *c->att;
  IpcShared::Pub& P = A.shm->pub[c->rank];
  // (pointer AND capacity: comm_reserve frees and allocates, and the allocator likes to hand the same address back for the
  //  larger buffer -- peers would go on copying through their mapping of the freed one.  Round-3 advisor finding.)
  if(R.send[cur] && (A.send_exported[cur] != (void*)R.send[cur].get() || A.send_exported_cap[cur] != R.send[cur].cap())) {
    if(hipIpcGetMemHandle(&P.send[cur], R.send[cur].get()) != hipSuccess) return ipc_fail(c, "hipIpcGetMemHandle");
    A.send_exported[cur] = R.send[cur].get(); A.send_exported_cap[cur] = R.send[cur].cap();
    P.send_epoch[cur] = ++A.send_epoch[cur];
  }
  return JFGPU_OK;
}

// Peer p's send buffer of turn `cur`, mapped into this process.
int ipc_peer_send(jfgpu_comm* c, int p, int cur, uint8_t** out) {
  IpcAttachment::PeerMap& M = c->att->peer_send[cur][p];
  const IpcShared::Pub& P = c->att->shm->pub[p];
  if(M.epoch != P.send_epoch[cur]) {
    if(M.ptr) { if(c->tun.comm_ipc_keep) c->att->stale_maps.push_back(M.ptr); else hipIpcCloseMemHandle(M.ptr); M.ptr = nullptr; }
    if(hipIpcOpenMemHandle(&M.ptr, P.send[cur], hipIpcMemLazyEnablePeerAccess) != hipSuccess) return ipc_fail(c, "hipIpcOpenMemHandle");
    M.epoch = P.send_epoch[cur];
  }
  *out = reinterpret_cast<uint8_t*>(M.ptr);
  return JFGPU_OK;
}

// Map every peer's send buffer of turn `cur` (only those re-allocated since they were last mapped), ONE RANK AT A TIME.
// Two processes importing each other's allocations at the same moment stalled in hipIpcOpenMemHandle for good with
// buffers of 2.6 GB and more (1.8 GB: fine; one process importing while the other idles: fine at any size,
// tools/probes/r03_ipc_size_probe.hip) -- so the imports take turns, with nothing of this exchange in flight yet.
int ipc_open_peers(jfgpu_comm* c, int cur) {
  for(int turn = 0; turn < c->world; ++turn) {
    int rc = JFGPU_OK;
    if(turn == c->rank)
      for(int p = 0; p < c->world && rc == JFGPU_OK; ++p) { uint8_t* unused; if(p != c->rank) rc = ipc_peer_send(c, p, cur, &unused); }
    if(rc) return rc;
    rc = ipc_barrier(c); if(rc) return rc;
  }
  return JFGPU_OK;
}

// Key path: every rank publishes its per-owner counts and offsets, then PULLS what is meant for it out of the peers'
// send buffers into its own receive buffer.
int comm_exchange_ipc(jfgpu_comm* c) {
  jfgpu_comm::Rank& R = c->ranks[0];
  const int cur = R.turn, W = c->world;
  IpcShared* shm = c->att->shm;
  IPC_TRACE(c, "keys: waiting for the routing kernels (turn %d)", cur);
  HIP_TRY(hipStreamSynchronize(R.t->stream));                // the routed keys are in send[cur]
  int rc = ipc_publish_send(c, cur); if(rc) return rc;
  IPC_TRACE(c, "keys: published, barrier 1");
  IpcShared::Pub& mine = shm->pub[c->rank];
  for(int p = 0; p < W; ++p) { mine.scount[p] = R.scount[cur][p]; mine.soff[p] = R.soff[cur][p]; }
  rc = ipc_barrier(c); if(rc) return rc;
  rc = ipc_open_peers(c, cur); if(rc) return rc;
  for(int p = 0; p < W; ++p) R.rcount[cur][p] = shm->pub[p].scount[c->rank];
  rc = comm_keys_recv_ready(c, R, false); if(rc) return rc;
  for(int p = 0; p < W; ++p) {
    if(!R.rcount[cur][p]) continue;
    uint8_t* src = reinterpret_cast<uint8_t*>(R.send[cur].get());
    if(p != c->rank) { rc = ipc_peer_send(c, p, cur, &src); if(rc) return rc; }
    HIP_TRY(hipMemcpyAsync(R.recv[cur] + R.roff[cur][p], src + shm->pub[p].soff[c->rank] * 8, R.rcount[cur][p] * 8, hipMemcpyDeviceToDevice, c->xstream));
  }
  HIP_TRY(hipEventRecord(R.exchanged[cur], c->xstream));
  IPC_TRACE(c, "keys: copies enqueued, waiting for them");
  HIP_TRY(hipStreamSynchronize(c->xstream));
  IPC_TRACE(c, "keys: pulled, barrier 2");
  rc = ipc_barrier(c); if(rc) return rc;                     // everybody has pulled: the send buffers may be written again
  IPC_TRACE(c, "keys: step exchanged");
  comm_free_retired(c, cur);                                 // (every peer has re-imported send[cur]: nobody maps the old ones)
  R.used[cur] = true;
  return JFGPU_OK;
}

// Item path: fixed layout, nothing to publish but the buffers.
int comm_exchange_items_ipc(jfgpu_comm* c) {
  jfgpu_comm::Rank& R = c->ranks[0];
  const int cur = R.turn, W = c->world, me = c->rank;
  const ItemLayout L = item_layout(c, R.t, R.icap[cur]);
  IPC_TRACE(c, "items: waiting for the routing kernels (turn %d, cap %u)", cur, R.icap[cur]);
  HIP_TRY(hipStreamSynchronize(R.t->stream));
  int rc = ipc_publish_send(c, cur); if(rc) return rc;
  IPC_TRACE(c, "items: published; waiting for recv[%d] to be consumed", cur);
  if(R.used[cur]) HIP_TRY(hipEventSynchronize(R.consumed[cur]));
  rc = comm_reserve(R.recv[cur], (L.recv_bytes + 7) / 8, R.t->stream, c->xstream); if(rc) return rc;
  IPC_TRACE(c, "items: recv buffer of %zu bytes ready, barrier 1", L.recv_bytes);
  rc = ipc_barrier(c); if(rc) return rc;
  rc = ipc_open_peers(c, cur); if(rc) return rc;
  IPC_TRACE(c, "items: peers' send buffers mapped");
  for(int p = 0; p < W; ++p) {                               // sender p's share for me
    uint8_t* sb = reinterpret_cast<uint8_t*>(R.send[cur].get());
    if(p != me) { rc = ipc_peer_send(c, p, cur, &sb); if(rc) return rc; }
    IPC_TRACE(c, "items: rank %d's send buffer is at %p here", p, (void*)sb);
    rc = comm_copy_share(c, L, R.recv[cur].get(), p, sb, me, true); if(rc) return rc;
  }
  HIP_TRY(hipEventRecord(R.exchanged[cur], c->xstream));
  IPC_TRACE(c, "items: copies enqueued, waiting for them");
  HIP_TRY(hipStreamSynchronize(c->xstream));
  IPC_TRACE(c, "items: pulled, barrier 2");
  rc = ipc_barrier(c); if(rc) return rc;
  IPC_TRACE(c, "items: step exchanged");
  comm_free_retired(c, cur);
  R.used[cur] = true;
  return JFGPU_OK;
}

int ipc_collective(jfgpu_comm* c, uint64_t* values, int n, int op /* 0 sum, 1 max, 2 gather of values[0] into values[0..world) */) {
  IpcShared* S = c->att->shm;
  for(int i = 0; i < (op == 2 ? 1 : n); ++i) S->coll[c->rank][i] = values[i];
  int rc = ipc_barrier(c); if(rc) return rc;
  if(op == 2) { for(int p = 0; p < c->world; ++p) values[p] = S->coll[p][0]; }
  else for(int i = 0; i < n; ++i) {
    uint64_t v = op == 0 ? 0 : S->coll[0][i];
    for(int p = 0; p < c->world; ++p) v = op == 0 ? v + S->coll[p][i] : std::max(v, S->coll[p][i]);
    values[i] = v;
  }
  return ipc_barrier(c);                                     // (the slots are free again)
}

// The communicator joins the block its id names.  Whatever fails from the mapping on, the attachment goes with the
// communicator and takes this rank's count out of the block again.
int ipc_attach(jfgpu_comm* c, const uint8_t* id128) {
  if(c->world > kIpcMaxWorld) return fail(JFGPU_E_INVALID, "ipc transport: at most 16 ranks");
  std::unique_ptr<IpcAttachment> A(new IpcAttachment);
  A->name.assign(reinterpret_cast<const char*>(id128) + 8);
  const int fd = shm_open(A->name.c_str(), O_CREAT | O_RDWR, 0600);           // created zero-filled by whoever comes first
  if(fd < 0) return fail(JFGPU_E_HIP, "ipc transport: shm_open failed");
  if(ftruncate(fd, sizeof(IpcShared)) != 0) { close(fd); return fail(JFGPU_E_HIP, "ipc transport: ftruncate failed"); }
  void* m = mmap(nullptr, sizeof(IpcShared), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  close(fd);
  if(m == MAP_FAILED) return fail(JFGPU_E_HIP, "ipc transport: mmap failed");
  A->shm = reinterpret_cast<IpcShared*>(m);
  A->shm->attached.fetch_add(1);
  for(int i = 0; i < 2; ++i) A->peer_send[i].assign(c->world, IpcAttachment::PeerMap());
  c->att = std::move(A);
  c->ipc = true;
  return ipc_barrier(c);                                     // everybody is here
}

// (the one-box test transport: importing a peer's send buffer of 10 GB never returned -- bench.py --gpus 2 --steps 4 on one
//  device, a 1.26 GB step as keys; 5 GB buffers are fine -- so such a step fails here, loudly and on every rank, instead
//  of standing in a barrier for ten minutes)
int ipc_keys_step_ok(jfgpu_comm* c, uint64_t send_bytes) {
  if(c->ipc && send_bytes > ((uint64_t)6 << 30))
    return ipc_fail(c, "a step of this size travels as keys in send buffers of more than 6 GiB, which this runtime does not import: feed smaller steps");
  return JFGPU_OK;
}

}  // namespace
#else
struct IpcAttachment {};
namespace {
int comm_exchange_ipc(jfgpu_comm*) { return fail(JFGPU_E_UNSUPPORTED, "no inter-process transport in the emulated build"); }
int comm_exchange_items_ipc(jfgpu_comm*) { return fail(JFGPU_E_UNSUPPORTED, "no inter-process transport in the emulated build"); }
int ipc_keys_step_ok(jfgpu_comm*, uint64_t) { return JFGPU_OK; }
}  // namespace
#endif
