// shard_xport.cpp — the shard's two transports and the creation of a handle
// over either: RCCL (one process per GPU, the product path), or an in-process
// group of P handles on one GPU whose collectives are device copies between
// the ranks' buffers (library-internal test hook: the routing logic of
// shard.cpp at P = 8 on the one GPU of a test box).
#include <rccl/rccl.h>
#include <string.h>

#include <condition_variable>
#include <mutex>

#include "shard_internal.h"

namespace {

int nccl_ok(ncclResult_t r, const char* what) {
  if (r == ncclSuccess) return SHM_OK;
  fprintf(stderr, "sherman_amd: %s failed: %s\n", what, ncclGetErrorString(r));
  return SHM_EIO;
}
#define NCCL_OK(expr)                                 \
  do {                                                \
    const int _rc = nccl_ok((expr), #expr);           \
    if (_rc) return _rc;                              \
  } while (0)

ncclDataType_t nccl_type(int eb) { return eb == 8 ? ncclUint64 : ncclUint32; }

struct RcclXport : Xport {
  ncclComm_t comm;
  bool own;
  RcclXport(ncclComm_t c, bool o) : comm(c), own(o) {}
  ~RcclXport() override {
    if (own && comm) (void)ncclCommDestroy(comm);
  }
  int group_start() override { return nccl_ok(ncclGroupStart(), "ncclGroupStart"); }
  int group_end() override { return nccl_ok(ncclGroupEnd(), "ncclGroupEnd"); }
  int a2a(const void* send, void* recv, uint64_t count, int eb, hipStream_t s) override {
    return nccl_ok(ncclAllToAll(send, recv, count, nccl_type(eb), comm, s), "ncclAllToAll");
  }
  int a2a_peers(const void* send, void* recv, uint64_t count, int eb, hipStream_t s) override {
    if ((P == 1 && !self_too) || count == 0) return SHM_OK;
    NCCL_OK(ncclGroupStart());
    for (uint32_t p = 0; p < P; ++p) {
      if (p == rank && !self_too) continue;
      NCCL_OK(ncclSend(static_cast<const char*>(send) + (uint64_t)p * count * eb, count,
                       nccl_type(eb), (int)p, comm, s));
      NCCL_OK(ncclRecv(static_cast<char*>(recv) + (uint64_t)p * count * eb, count, nccl_type(eb),
                       (int)p, comm, s));
    }
    NCCL_OK(ncclGroupEnd());
    return SHM_OK;
  }
  int p2p(const void* send, const uint64_t* scnt, const uint64_t* soff, void* recv,
          const uint64_t* rcnt, const uint64_t* roff, int eb, hipStream_t s) override {
    NCCL_OK(ncclGroupStart());
    for (uint32_t p = 0; p < P; ++p) {
      if (scnt[p])
        NCCL_OK(ncclSend(static_cast<const char*>(send) + soff[p] * eb, scnt[p], nccl_type(eb),
                         (int)p, comm, s));
      if (rcnt[p])
        NCCL_OK(ncclRecv(static_cast<char*>(recv) + roff[p] * eb, rcnt[p], nccl_type(eb), (int)p,
                         comm, s));
    }
    NCCL_OK(ncclGroupEnd());
    return SHM_OK;
  }
};

// In-process group of P ranks on one device, each driven by its own host
// thread (test hook).  A collective: every rank posts its buffers and an
// event recorded after their producers, a host barrier, every rank copies
// its parts out of the peers' send buffers on its stream (after their
// events), a barrier, every rank's stream waits for the peers' copies before
// its send buffer may change, a barrier before the posts are reused.
struct LocalGroup {
  uint32_t P;
  std::mutex mu;
  std::condition_variable cv;
  uint64_t gen = 0;
  uint32_t arrived = 0;
  struct Post {
    const char* send = nullptr;
    const uint64_t* scnt = nullptr;
    const uint64_t* soff = nullptr;
    uint64_t count = 0;
    hipEvent_t ready = nullptr, done = nullptr;
  };
  std::vector<Post> post;
  // point-to-point mailboxes [src * P + dst]: only the pairs with data meet
  // (as ncclSend / ncclRecv), so a rank with nothing to exchange skips it
  struct Mail {
    const char* send = nullptr;
    uint64_t bytes = 0;
    hipEvent_t ready = nullptr;  // sender: its data produced
    hipEvent_t done = nullptr;   // receiver: its copy queued
    int state = 0;               // 0 empty, 1 posted, 2 consumed
  };
  std::vector<Mail> mail;
  explicit LocalGroup(uint32_t p) : P(p), post(p), mail((size_t)p * p) {}
  void barrier() {
    std::unique_lock<std::mutex> lk(mu);
    const uint64_t g = gen;
    if (++arrived == P) {
      arrived = 0;
      ++gen;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return gen != g; });
    }
  }
};

struct LocalXport : Xport {
  LocalGroup* g;
  DevEvent ready, done;
  std::vector<DevEvent> sev, rev;  // per peer: p2p send-ready / receive-done
  explicit LocalXport(LocalGroup* grp) : g(grp), sev(grp->P), rev(grp->P) {}
  int init() {
    RC_OK(ready.create());
    RC_OK(done.create());
    for (uint32_t p = 0; p < g->P; ++p) {
      RC_OK(sev[p].create());
      RC_OK(rev[p].create());
    }
    return SHM_OK;
  }
  // copy(p) enqueues the part from peer p; then the hand-back protocol
  template <class F>
  int run(const LocalGroup::Post& mine, hipStream_t s, F copy) {
    int rc = SHM_OK;
    if (hipEventRecord(ready, s) != hipSuccess) rc = SHM_EIO;
    LocalGroup::Post m = mine;
    m.ready = ready;
    m.done = done;
    g->post[rank] = m;
    g->barrier();
    for (uint32_t p = 0; p < P; ++p) {
      if (hipStreamWaitEvent(s, g->post[p].ready, 0) != hipSuccess) rc = SHM_EIO;
      if (copy(p, g->post[p])) rc = SHM_EIO;
    }
    if (hipEventRecord(done, s) != hipSuccess) rc = SHM_EIO;
    g->barrier();
    for (uint32_t p = 0; p < P; ++p)
      if (hipStreamWaitEvent(s, g->post[p].done, 0) != hipSuccess) rc = SHM_EIO;
    g->barrier();
    return rc;
  }
  int a2a(const void* send, void* recv, uint64_t count, int eb, hipStream_t s) override {
    LocalGroup::Post m;
    m.send = static_cast<const char*>(send);
    m.count = count;
    return run(m, s, [&](uint32_t p, const LocalGroup::Post& q) {
      if (!count) return 0;
      return hipMemcpyAsync(static_cast<char*>(recv) + (uint64_t)p * count * eb,
                            q.send + (uint64_t)rank * count * eb, count * eb,
                            hipMemcpyDeviceToDevice, s) != hipSuccess ? 1 : 0;
    });
  }
  int a2a_peers(const void* send, void* recv, uint64_t count, int eb, hipStream_t s) override {
    LocalGroup::Post m;
    m.send = static_cast<const char*>(send);
    m.count = count;
    return run(m, s, [&](uint32_t p, const LocalGroup::Post& q) {
      if (!count || (p == rank && !self_too)) return 0;
      return hipMemcpyAsync(static_cast<char*>(recv) + (uint64_t)p * count * eb,
                            q.send + (uint64_t)rank * count * eb, count * eb,
                            hipMemcpyDeviceToDevice, s) != hipSuccess ? 1 : 0;
    });
  }
  // post every send, take every receive, then wait until the sends were taken
  // (no rank blocks before all of its sends are posted: no cycle)
  int p2p(const void* send, const uint64_t* scnt, const uint64_t* soff, void* recv,
          const uint64_t* rcnt, const uint64_t* roff, int eb, hipStream_t s) override {
    const uint32_t P = g->P;
    int rc = SHM_OK;
    std::unique_lock<std::mutex> lk(g->mu);
    for (uint32_t p = 0; p < P; ++p) {
      if (!scnt[p]) continue;
      LocalGroup::Mail& m = g->mail[(size_t)rank * P + p];
      g->cv.wait(lk, [&] { return m.state == 0; });
      if (hipEventRecord(sev[p], s) != hipSuccess) rc = SHM_EIO;
      m.send = static_cast<const char*>(send) + soff[p] * eb;
      m.bytes = scnt[p] * eb;
      m.ready = sev[p];
      m.state = 1;
    }
    g->cv.notify_all();
    for (uint32_t p = 0; p < P; ++p) {
      if (!rcnt[p]) continue;
      LocalGroup::Mail& m = g->mail[(size_t)p * P + rank];
      g->cv.wait(lk, [&] { return m.state == 1; });
      if (m.bytes != rcnt[p] * eb) rc = SHM_EIO;  // the two sides disagree on a count
      if (hipStreamWaitEvent(s, m.ready, 0) != hipSuccess ||
          hipMemcpyAsync(static_cast<char*>(recv) + roff[p] * eb, m.send,
                         std::min<uint64_t>(m.bytes, rcnt[p] * eb), hipMemcpyDeviceToDevice,
                         s) != hipSuccess ||
          hipEventRecord(rev[p], s) != hipSuccess)
        rc = SHM_EIO;
      m.done = rev[p];
      m.state = 2;
      g->cv.notify_all();
    }
    for (uint32_t p = 0; p < P; ++p) {
      if (!scnt[p]) continue;
      LocalGroup::Mail& m = g->mail[(size_t)rank * P + p];
      g->cv.wait(lk, [&] { return m.state == 2; });
      // the receiver's copy out of our buffer precedes anything we queue next
      if (hipStreamWaitEvent(s, m.done, 0) != hipSuccess) rc = SHM_EIO;
      m.state = 0;
    }
    g->cv.notify_all();
    return rc;
  }
};

int rccl_shard(shm_tree* local, ncclComm_t comm, uint32_t world, uint32_t rank, bool own,
               shm_shard** out) {
  // two more communicators split from the first (same ranks, same order), so
  // the two search slots and the exclusive calls never serialise on one; a
  // failed split leaves through the transports made so far, last to first
  std::unique_ptr<Xport> x[3];
  x[0].reset(new RcclXport(comm, own));
  for (int i = 1; i < 3; ++i) {
    ncclComm_t c = nullptr;
    if (nccl_ok(ncclCommSplit(comm, 0, (int)rank, &c, nullptr), "ncclCommSplit") || !c)
      return SHM_EIO;
    x[i].reset(new RcclXport(c, true));
  }
  return make_shard(local, x, world, rank, out);
}

}  // namespace

extern "C" {

int shm_nccl_unique_id(void* id_out, uint64_t bytes) {
  if (!id_out || bytes < sizeof(ncclUniqueId)) return SHM_EINVAL;
  ncclUniqueId id;
  NCCL_OK(ncclGetUniqueId(&id));
  memcpy(id_out, &id, sizeof(id));
  return SHM_OK;
}

int shm_shard_create(shm_tree* local, const void* nccl_id, uint64_t id_bytes, uint32_t world,
                     uint32_t rank, shm_shard** out) {
  if (!local || !nccl_id || id_bytes < sizeof(ncclUniqueId) || !out || world == 0 ||
      world > kMaxWorld || rank >= world)
    return SHM_EINVAL;
  ncclUniqueId id;
  memcpy(&id, nccl_id, sizeof(id));
  ncclComm_t comm = nullptr;
  NCCL_OK(ncclCommInitRank(&comm, (int)world, id, (int)rank));
  return rccl_shard(local, comm, world, rank, true, out);
}

int shm_shard_create_with_comm(shm_tree* local, void* nccl_comm, uint32_t world, uint32_t rank,
                               shm_shard** out) {
  if (!local || !nccl_comm || !out || world == 0 || world > kMaxWorld || rank >= world)
    return SHM_EINVAL;
  return rccl_shard(local, (ncclComm_t)nccl_comm, world, rank, false, out);
}

// Library-internal test hooks, not part of include/sherman_amd.h: an
// in-process group of P shard handles on one device (P trees, one host
// thread per rank, every rank's calls on ONE shared stream so the trees'
// persistent kernels never share the device): the whole routed path —
// slots, overflow rounds, padded inserts and their tails, range pieces — with
// device copies for the collectives (tests/test_gpu_shard_local.py at P = 8).
int shm__local_group_create(uint32_t world, void** out) {
  if (!out || world == 0 || world > kMaxWorld) return SHM_EINVAL;
  *out = new LocalGroup(world);
  return SHM_OK;
}
int shm__local_group_destroy(void* g) {
  delete static_cast<LocalGroup*>(g);
  return SHM_OK;
}
int shm__shard_create_local(shm_tree* local, void* group, uint32_t rank, shm_shard** out) {
  LocalGroup* g = static_cast<LocalGroup*>(group);
  if (!local || !g || !out || rank >= g->P) return SHM_EINVAL;
  std::unique_ptr<Xport> x[3];
  for (auto& xi : x) {
    LocalXport* lx = new LocalXport(g);
    xi.reset(lx);
    if (lx->init()) return SHM_EIO;
  }
  return make_shard(local, x, g->P, rank, out);
}

}  // extern "C"
