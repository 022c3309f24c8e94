// dx_comm.hip -- multi-GPU observation collation: RCCL (librccl) directly, no framework
// layer.  One process per GPU.  Physics has no exchange (environments are independent);
// the only collective is the per-control-step all-gather of the packed outputs,
// enqueued on the env's stream right behind the task post kernel, so the host
// never waits for it.  The gather is in place: this rank packs straight into its
// own slice of dst.
#include <rccl/rccl.h>

#include "dx_host.h"

struct dx_comm {
  ncclComm_t comm = nullptr;
  int rank = 0, nranks = 1, device = 0;
  hipStream_t stream = nullptr;  // barrier / scalar reductions
  double* scalar = nullptr;      // device scratch for dx_comm_allreduce_max
};

#define NCCLCHK(x)                                                                                 \
  do {                                                                                             \
    ncclResult_t r_ = (x);                                                                         \
    if (r_ != ncclSuccess) return dx_fail(DX_EHIP, std::string(#x ": ") + ncclGetErrorString(r_));    \
  } while (0)

extern "C" int dx_comm_unique_id(void* id) {
  if (!id) return dx_fail(DX_EINVAL, "null id buffer");
  static_assert(sizeof(ncclUniqueId) == DX_COMM_ID_BYTES, "RCCL unique id size");
  ncclUniqueId u;
  NCCLCHK(ncclGetUniqueId(&u));
  memcpy(id, &u, sizeof(u));
  return 0;
}

extern "C" dx_comm* dx_comm_init(const void* id, int32_t nranks, int32_t rank, int32_t device) {
  if (!id || nranks < 1 || rank < 0 || rank >= nranks) { dx_fail(DX_EINVAL, "bad comm arguments"); return nullptr; }
  if (hipSetDevice(device) != hipSuccess) { dx_fail(DX_EHIP, "hipSetDevice failed"); return nullptr; }
  dx_comm* c = new dx_comm();
  c->rank = rank;
  c->nranks = nranks;
  c->device = device;
  ncclUniqueId u;
  memcpy(&u, id, sizeof(u));
  ncclResult_t r = ncclCommInitRank(&c->comm, nranks, u, rank);
  if (r != ncclSuccess) {
    dx_fail(DX_EHIP, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    delete c;
    return nullptr;
  }
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc(&c->scalar, sizeof(double)) != hipSuccess) {
    dx_fail(DX_EHIP, "comm stream / scratch allocation failed");
    dx_comm_destroy(c);
    return nullptr;
  }
  return c;
}

extern "C" void dx_comm_destroy(dx_comm* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm) (void)ncclCommDestroy(c->comm);
  if (c->scalar) (void)hipFree(c->scalar);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

extern "C" int dx_comm_rank(const dx_comm* c) { return c ? c->rank : dx_fail(DX_EINVAL, "null comm"); }
extern "C" int dx_comm_size(const dx_comm* c) { return c ? c->nranks : dx_fail(DX_EINVAL, "null comm"); }

extern "C" int dx_allgather_obs(dx_env* e, dx_comm* c, float* dst_dev) {
  if (!e || !c || !dst_dev) return dx_fail(DX_EINVAL, "null argument");
  dx_batch* b = e->batch;
  if (b->device != c->device) return dx_fail(DX_EINVAL, "env and comm are on different devices");
  const size_t count = (size_t)e->P.nenv * (e->P.obs_dim + 3);
  float* mine = dst_dev + (size_t)c->rank * count;
  if (int rc = dx_env_pack_outputs(e, mine)) return rc;
  NCCLCHK(ncclAllGather(mine, dst_dev, count, ncclFloat32, c->comm, b->stream));
  return 0;
}

extern "C" int dx_comm_allreduce_max(dx_comm* c, double* value) {
  if (!c || !value) return dx_fail(DX_EINVAL, "null argument");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(c->scalar, value, sizeof(double), hipMemcpyHostToDevice, c->stream));
  NCCLCHK(ncclAllReduce(c->scalar, c->scalar, 1, ncclFloat64, ncclMax, c->comm, c->stream));
  HIPCHK(hipMemcpyAsync(value, c->scalar, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int dx_comm_barrier(dx_comm* c) {
  double x = 0;
  return dx_comm_allreduce_max(c, &x);
}
