// comm.hip — the communicators of a context: the lazily bound RCCL table, the in-process stand-in of the tests, the two collectives
// every solve path calls (allreduce, broadcast) and the pmpc_comm_* entries of include/pmpc_abi.h.
#include "solver_internal.h"

namespace {

// ---- lazily bound RCCL (the library must load on machines where no communicator is ever made) ----
struct Rccl {
  void *h = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Broadcast)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  bool load() {
    if (h) return true;
    const char *names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};  // torch bundles soname librccl.so: reuse the loaded copy
    for (const char *n : names)
      if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) return false;
    GetUniqueId = (decltype(GetUniqueId))dlsym(h, "ncclGetUniqueId");
    CommInitRank = (decltype(CommInitRank))dlsym(h, "ncclCommInitRank");
    CommDestroy = (decltype(CommDestroy))dlsym(h, "ncclCommDestroy");
    AllReduce = (decltype(AllReduce))dlsym(h, "ncclAllReduce");
    Broadcast = (decltype(Broadcast))dlsym(h, "ncclBroadcast");
    return GetUniqueId && CommInitRank && AllReduce && Broadcast;
  }
};
Rccl g_rccl;

// ---- in-process communicator (TEST HOOK, pmpc_comm_init_mock) --------------------------------------------------------
// RCCL refuses two ranks on one device, so on a single-GPU box the world > 1 code paths (packed scalar exchange, consensus
// all-reduce, owner / bounds broadcast) could never run.  This stand-in lets N contexts on ONE device, each driven by its
// own host thread, play the ranks: a collective synchronises the caller's stream, meets the other ranks at a barrier,
// reduces on the host in rank order and writes the result back.  Same call signature as the RCCL entry points it
// replaces; correctness only, no performance meaning.
struct MockGroup {
  int world = 0, arrived = 0, generation = 0;
  std::mutex m;
  std::condition_variable cv;
  std::vector<std::vector<unsigned char>> slot;  // one staging buffer per rank
  void barrier() {
    std::unique_lock<std::mutex> lk(m);
    const int gen = generation;
    if (++arrived == world) { arrived = 0; generation++; cv.notify_all(); }
    else cv.wait(lk, [&] { return gen != generation; });
  }
};
struct MockRank { MockGroup *g; int rank; };
std::map<int, MockGroup *> g_mock_groups;
std::mutex g_mock_mutex;

template <class T>
void mock_reduce(MockGroup *g, size_t n, ncclRedOp_t op, T *out) {
  for (size_t k = 0; k < n; k++) {
    T acc = ((const T *)g->slot[0].data())[k];
    for (int r = 1; r < g->world; r++) {
      const T v = ((const T *)g->slot[r].data())[k];
      acc = op == ncclSum ? (T)(acc + v) : (op == ncclMin ? std::min(acc, v) : std::max(acc, v));
    }
    out[k] = acc;
  }
}
ncclResult_t mock_allreduce(const void *send, void *recv, size_t n, ncclDataType_t dt, ncclRedOp_t op, ncclComm_t comm, hipStream_t s) {
  MockRank *mr = (MockRank *)comm;
  MockGroup *g = mr->g;
  const size_t esz = dt == ncclFloat64 ? 8 : 4;
  HIP_CHECK(hipStreamSynchronize(s));
  g->slot[mr->rank].resize(n * esz);
  HIP_CHECK(hipMemcpy(g->slot[mr->rank].data(), send, n * esz, hipMemcpyDeviceToHost));
  g->barrier();
  std::vector<unsigned char> out(n * esz);
  if (dt == ncclFloat64) mock_reduce<double>(g, n, op, (double *)out.data());
  else mock_reduce<int>(g, n, op, (int *)out.data());
  g->barrier();  // everyone has read the slots before anyone overwrites them in the next collective
  HIP_CHECK(hipMemcpy(recv, out.data(), n * esz, hipMemcpyHostToDevice));
  return ncclSuccess;
}
ncclResult_t mock_broadcast(const void *send, void *recv, size_t n, ncclDataType_t dt, int root, ncclComm_t comm, hipStream_t s) {
  MockRank *mr = (MockRank *)comm;
  MockGroup *g = mr->g;
  const size_t esz = dt == ncclFloat64 ? 8 : 4;
  HIP_CHECK(hipStreamSynchronize(s));
  if (mr->rank == root) {
    g->slot[root].resize(n * esz);
    HIP_CHECK(hipMemcpy(g->slot[root].data(), send, n * esz, hipMemcpyDeviceToHost));
  }
  g->barrier();
  std::vector<unsigned char> out(g->slot[root].begin(), g->slot[root].begin() + n * esz);
  g->barrier();
  HIP_CHECK(hipMemcpy(recv, out.data(), n * esz, hipMemcpyHostToDevice));
  return ncclSuccess;
}

}  // namespace

namespace pmpc_impl {

void allreduce(pmpc_ctx *c, void *buf, size_t n, ncclDataType_t dt, ncclRedOp_t op) {
  if (!c->multi()) return;
  ncclResult_t r = g_rccl.AllReduce(buf, buf, n, dt, op, c->comm, c->stream);
  if (r != ncclSuccess) {
    fprintf(stderr, "pmpc_hip: ncclAllReduce failed (%d)\n", (int)r);
    throw PmpcHipError{(int)r, "ncclAllReduce", __FILE__, __LINE__};
  }
}
void broadcast(pmpc_ctx *c, void *buf, size_t n, ncclDataType_t dt, int root) {
  ncclResult_t r = g_rccl.Broadcast(buf, buf, n, dt, root, c->comm, c->stream);
  if (r != ncclSuccess) {
    fprintf(stderr, "pmpc_hip: ncclBroadcast failed (%d)\n", (int)r);
    throw PmpcHipError{(int)r, "ncclBroadcast", __FILE__, __LINE__};
  }
}
void comm_release(pmpc_ctx *c) {  // pmpc_destroy's share: the context's communicator, whichever kind it is
  if (c->comm && c->mock_comm) delete (MockRank *)c->comm;
  else if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
}

}  // namespace pmpc_impl

extern "C" {

int pmpc_comm_unique_id(void *out128) {
  if (!g_rccl.load()) return 1;
  ncclUniqueId id;
  if (g_rccl.GetUniqueId(&id) != ncclSuccess) return 2;
  memcpy(out128, &id, sizeof(id));
  return 0;
}

int pmpc_comm_init(pmpc_ctx *c, int rank, int world, const void *id128) {
  // TEST HOOK: PMPC_RCCL_SINGLE=1 makes a world of one a real 1-rank RCCL communicator and sends every solve through the
  // multi-rank code paths (packed exchange, consensus all-reduce, bounds broadcast) — the only way to run the actual
  // ncclAllReduce / ncclBroadcast calls on a one-GPU box (RCCL refuses two ranks on one device).
  const char *single = getenv("PMPC_RCCL_SINGLE");
  if (world <= 1 && !(single && single[0] == '1')) {
    c->rank = 0;
    c->world = 1;
    return 0;
  }
  if (world <= 1) { world = 1; rank = 0; c->single_rank_comm = true; }
  if (!g_rccl.load()) return 1;
  if (hipSetDevice(c->device) != hipSuccess) return 3;
  ncclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  if (g_rccl.CommInitRank(&c->comm, world, id, rank) != ncclSuccess) return 2;
  c->rank = rank;
  c->world = world;
  return 0;
}
// TEST HOOK: join the in-process communicator `group` (see MockGroup above) as rank `rank` of `world`.  Every context of
// the group lives on one device and must be driven by its own host thread.  Installs the stand-in collectives
// process-wide: do not mix with a real RCCL communicator in the same process.
int pmpc_comm_init_mock(pmpc_ctx *c, int rank, int world, int group) {
  std::lock_guard<std::mutex> lk(g_mock_mutex);
  MockGroup *&g = g_mock_groups[group];
  if (!g) {
    g = new MockGroup();
    g->world = world;
    g->slot.resize(world);
  }
  if (g->world != world || rank < 0 || rank >= world) return 1;
  g_rccl.AllReduce = mock_allreduce;
  g_rccl.Broadcast = mock_broadcast;
  c->comm = (ncclComm_t) new MockRank{g, rank};
  c->mock_comm = true;
  c->rank = rank;
  c->world = world;
  return 0;
}

}  // extern "C"
