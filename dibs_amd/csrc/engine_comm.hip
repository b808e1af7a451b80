// In-engine exchange of a particle-sharded run (include/dibs_hip.h): RCCL bound at run time or mapped peer memory (exchange_ipc.h, whose
// kernels are compiled here), and the step loop of a sharded chunk.
#define DIBS_TU_COMM
#include "engine_impl.h"
#include <dlfcn.h>
#include <unistd.h>

// ---- in-engine exchange: RCCL bound at run time, the step loop of a sharded run in C (include/dibs_hip.h) ---------------------------------
// librccl.so.1 is dlopen'ed on first use: in a process that has imported torch this is torch's bundled copy (same SONAME, already
// mapped), otherwise ROCm's -- one RCCL per process either way, and libdibs_hip.so loads on machines without it.
struct dibs_rccl {
  decltype(&ncclGetUniqueId) get_unique_id = nullptr;
  decltype(&ncclCommInitRank) comm_init_rank = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclAllGather) all_gather = nullptr;
  decltype(&ncclGetErrorString) error_string = nullptr;
  bool ok = false;
  std::string why;
};
static const dibs_rccl& rccl() {
  static const dibs_rccl r = [] {
    dibs_rccl q;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
      q.why = std::string("librccl not found: ") + dlerror();
      return q;
    }
    q.get_unique_id = (decltype(q.get_unique_id))dlsym(h, "ncclGetUniqueId");
    q.comm_init_rank = (decltype(q.comm_init_rank))dlsym(h, "ncclCommInitRank");
    q.comm_destroy = (decltype(q.comm_destroy))dlsym(h, "ncclCommDestroy");
    q.all_gather = (decltype(q.all_gather))dlsym(h, "ncclAllGather");
    q.error_string = (decltype(q.error_string))dlsym(h, "ncclGetErrorString");
    q.ok = q.get_unique_id && q.comm_init_rank && q.comm_destroy && q.all_gather && q.error_string;
    if (!q.ok) q.why = "librccl lacks one of ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllGather / ncclGetErrorString";
    return q;
  }();
  return r;
}
#define RCCL_OK(expr)                                                                                    \
  do {                                                                                                   \
    ncclResult_t _r = (expr);                                                                            \
    if (_r != ncclSuccess) return fail(std::string(#expr) + ": " + rccl().error_string(_r));             \
  } while (0)

static_assert(DIBS_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "include/dibs_hip.h: DIBS_COMM_ID_BYTES");

extern "C" int dibs_comm_unique_id(void* id_out) {
  if (!id_out) return fail("null argument");
  if (!rccl().ok) return fail(rccl().why);
  ncclUniqueId id;
  RCCL_OK(rccl().get_unique_id(&id));
  memcpy(id_out, id.internal, NCCL_UNIQUE_ID_BYTES);
  return 0;
}

extern "C" int dibs_engine_comm_destroy(dibs_engine* e) {
  if (!e) return 0;
  for (int i = 0; i < 2; ++i)
    if (e->comm[i]) {
      rccl().comm_destroy(e->comm[i]);
      e->comm[i] = nullptr;
    }
  e->n_comms = 0;
  if (e->agree_dev) hipFree(e->agree_dev);
  if (e->agree_host) hipHostFree(e->agree_host);
  e->agree_dev = e->agree_host = nullptr;
  if (e->ipc.arena || e->ipc.err) {
    // (the peers must have left their last exchange: every rank returns from dibs_engine_run_sharded / gather_particles only after it has seen
    //  all of its peers' rows, and nobody writes into an arena outside an exchange)
    for (int r = 0; r < IPC_MAX_RANKS; ++r)
      if (e->ipc.opened[r]) hipIpcCloseMemHandle(e->ipc.peers.base[r]);
    if (e->ipc.arena) hipFree(e->ipc.arena);
    if (e->ipc.err) hipHostFree(e->ipc.err);
    e->ipc = IpcComm{};
  }
  if (e->planes) hipFree(e->planes);
  if (e->vsend) hipFree(e->vsend);
  e->planes = e->vsend = nullptr;
  if (e->side) hipStreamDestroy(e->side);
  if (e->ev_exported) hipEventDestroy(e->ev_exported);
  if (e->ev_vals) hipEventDestroy(e->ev_vals);
  e->side = nullptr;
  e->ev_exported = e->ev_vals = nullptr;
  return 0;
}

extern "C" int dibs_engine_comm_init(dibs_engine* e, const void* ids, int32_t n_ids) {
  if (!e) return fail("null argument");
  if (refuse_chains(e, "the sharded entry points (chains are not sharded over ranks)")) return 1;
  if (e->B > 1) return fail("batched engine: a batch is not sharded over ranks");
  if (n_ids < 1 || n_ids > 2) return fail("n_ids must be 1 (one all-gather per step) or 2 (overlapped exchange as well)");
  // ids == NULL: LOOPBACK -- no communicator, the all-gathers are skipped and the rows of the other ranks keep whatever the buffers hold.
  // A measuring device (scripts/gpu_shard_scaling.py: what ONE rank of an N-way run costs per step in this loop, on one GPU), not a
  // way to run a sharded job.
  if (ids && !rccl().ok) return fail(rccl().why);
  HIP_OK(hipSetDevice(e->cfg.device_id));
  dibs_engine_comm_destroy(e);
  e->loopback = ids == nullptr;
  for (int i = 0; ids && i < n_ids; ++i) {
    ncclUniqueId id;
    memcpy(id.internal, (const char*)ids + (size_t)i * NCCL_UNIQUE_ID_BYTES, NCCL_UNIQUE_ID_BYTES);
    RCCL_OK(rccl().comm_init_rank(&e->comm[i], e->cfg.n_ranks, id, e->cfg.rank));
  }
  e->n_comms = n_ids;
  HIP_OK(dalloc(&e->agree_dev, (size_t)4 + 4 * e->cfg.n_ranks));
  HIP_OK(hipHostMalloc((void**)&e->agree_host, ((size_t)4 + 4 * e->cfg.n_ranks) * 4, hipHostMallocDefault));
  if (n_ids == 2) {
    HIP_OK(dalloc(&e->planes, (size_t)2 * e->M * e->Ev));
    HIP_OK(dalloc(&e->vsend, (size_t)e->Mloc * e->Ev));
    HIP_OK(hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking));
    HIP_OK(hipEventCreateWithFlags(&e->ev_exported, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&e->ev_vals, hipEventDisableTiming));
    HIP_OK(hipDeviceSynchronize());
  }
  e->vals_fresh = false;
  return 0;
}

// ---- the exchange through mapped peer memory (exchange_ipc.h): ranks that share a device, or devices with peer access ------------------
static_assert(DIBS_IPC_HANDLE_BYTES == sizeof(IpcBlob), "include/dibs_hip.h: DIBS_IPC_HANDLE_BYTES");

// allocates this rank's exchange arena (zeroed: no exchange has arrived) and writes the blob its peers need to map it
extern "C" int dibs_engine_ipc_export(dibs_engine* e, void* blob_out) {
  if (!e || !blob_out) return fail("null argument");
  if (refuse_chains(e, "the sharded entry points (chains are not sharded over ranks)")) return 1;
  if (e->B > 1) return fail("batched engine: a batch is not sharded over ranks");
  if (e->cfg.n_ranks > IPC_MAX_RANKS) return fail("the mapped-memory exchange supports at most " + std::to_string(IPC_MAX_RANKS) + " ranks");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  dibs_engine_comm_destroy(e);
  IpcComm& c = e->ipc;
  c.n_ranks = e->cfg.n_ranks;
  c.rank = e->cfg.rank;
  c.pack_elems = (size_t)e->M * e->E;
  c.set_elems = (size_t)2 * e->M * e->Ev;
  c.arena_bytes = IPC_FLAG_BYTES + (2 * c.pack_elems + 2 * c.set_elems) * 4;
  HIP_OK(hipMalloc((void**)&c.arena, c.arena_bytes));
  HIP_OK(hipMemset(c.arena, 0, c.arena_bytes));
  HIP_OK(hipDeviceSynchronize());
  IpcBlob b;
  memset(&b, 0, sizeof b);
  b.magic = IPC_MAGIC;
  b.abi = DIBS_ABI_VERSION;
  b.rank = (uint32_t)c.rank;
  b.n_ranks = (uint32_t)c.n_ranks;
  b.arena_bytes = c.arena_bytes;
  b.pack_elems = c.pack_elems;
  b.set_elems = c.set_elems;
  b.device_id = e->cfg.device_id;
  b.pid = (int32_t)getpid();
  HIP_OK(hipIpcGetMemHandle(&b.handle, c.arena));
  memcpy(blob_out, &b, sizeof b);
  return 0;
}

// blobs_all: the n_ranks blobs of dibs_engine_ipc_export in rank order (every rank passes the same bytes)
extern "C" int dibs_engine_comm_init_ipc(dibs_engine* e, const void* blobs_all) {
  if (!e || !blobs_all) return fail("null argument");
  IpcComm& c = e->ipc;
  if (!c.arena) return fail("dibs_engine_ipc_export has not been called on this engine");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  const IpcBlob* B = reinterpret_cast<const IpcBlob*>(blobs_all);
  for (int r = 0; r < c.n_ranks; ++r) {
    IpcBlob b;
    memcpy(&b, B + r, sizeof b);
    if (b.magic != IPC_MAGIC || b.abi != DIBS_ABI_VERSION) return fail("blob of rank " + std::to_string(r) + ": not a dibs_engine_ipc_export blob of this ABI version");
    if ((int)b.rank != r || (int)b.n_ranks != c.n_ranks) return fail("blob " + std::to_string(r) + " belongs to rank " + std::to_string(b.rank) + " of " + std::to_string(b.n_ranks));
    if (b.arena_bytes != c.arena_bytes || b.pack_elems != c.pack_elems || b.set_elems != c.set_elems)
      return fail("rank " + std::to_string(r) + " was created with a different configuration (exchange arena sizes differ)");
    if (r == c.rank) {
      c.peers.base[r] = c.arena;
      continue;
    }
    if (b.pid == (int32_t)getpid()) return fail("the mapped-memory exchange needs one PROCESS per rank (rank " + std::to_string(r) + " lives in this process)");
    void* p = nullptr;
    HIP_OK(hipIpcOpenMemHandle(&p, b.handle, hipIpcMemLazyEnablePeerAccess));
    c.peers.base[r] = (char*)p;
    c.opened[r] = true;
  }
  HIP_OK(hipHostMalloc((void**)&c.err, 4, hipHostMallocDefault));
  *c.err = 0u;
  if (e->tune.ipc_timeout_ms > 0) c.wait_ticks = (unsigned long long)e->tune.ipc_timeout_ms * 100000ull;  // (100 MHz ticks; tuning.h)
  HIP_OK(dalloc(&e->agree_dev, (size_t)4 + 4 * e->cfg.n_ranks));
  HIP_OK(hipHostMalloc((void**)&e->agree_host, ((size_t)4 + 4 * e->cfg.n_ranks) * 4, hipHostMallocDefault));
  HIP_OK(dalloc(&e->vsend, (size_t)e->Mloc * e->Ev));
  HIP_OK(hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking));
  HIP_OK(hipEventCreateWithFlags(&e->ev_exported, hipEventDisableTiming));
  HIP_OK(hipEventCreateWithFlags(&e->ev_vals, hipEventDisableTiming));
  HIP_OK(hipDeviceSynchronize());
  c.on = true;
  e->loopback = false;
  e->n_comms = 2;  // (both protocols: the arena holds the packed rows and the planes)
  e->vals_fresh = false;
  return 0;
}

// one all-gather through the arenas on stream `st`: `n` floats at `src` (this rank's rows) -> byte offset dst_off of every peer's arena
// (include_self: and of the own one), then the announcement + wait of this exchange on `channel`
static int ipc_all_gather(dibs_engine* e, int channel, hipStream_t st, const float* src, size_t dst_off, size_t n, bool include_self) {
  IpcComm& c = e->ipc;
  if ((n & 3) || (dst_off & 15) || (reinterpret_cast<uintptr_t>(src) & 15)) return fail("internal: exchange rows are not 16-byte aligned");
  const size_t n4 = n / 4;
  const int ndst = include_self ? c.n_ranks : c.n_ranks - 1;
  if (ndst > 0 && n4 > 0) {
    const unsigned bx = (unsigned)((n4 + 255) / 256 < 256 ? (n4 + 255) / 256 : 256);
    hipLaunchKernelGGL(k_ipc_push, dim3(bx, (unsigned)ndst), dim3(256), 0, st, c.peers, c.rank, c.n_ranks, include_self ? 1 : 0,
                       reinterpret_cast<const float4*>(src), dst_off, n4);
  }
  const unsigned int seq = ++c.seq[channel];
  if (c.n_ranks > 1) hipLaunchKernelGGL(k_ipc_signal_wait, dim3(1), dim3(64), 0, st, c.peers, c.rank, c.n_ranks, channel, seq, c.wait_ticks, c.err);
  HIP_OK(hipGetLastError());
  return 0;
}

// Loopback stand-in for the all-gather of the values (per-rank timing on one GPU).  A plain copy KERNEL: hipMemcpyAsync(DeviceToDevice) on the
// side stream made the un-profiled loop of a 4-way rank take 380 us per step instead of 103 (and 107 under rocprofv3, which turns the copy
// into a blit kernel): the runtime's copy path resolves the cross-stream dependency on the host.  RCCL's all-gather is a kernel as well.
__global__ void k_copy_rows(const float4* __restrict__ src, float4* __restrict__ dst, size_t n4) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n4) dst[i] = src[i];
}

// values of this rank (already in vsend unless `exported`) -> plane 0 of every rank on the side stream, kernel slab behind the gather
static int exchange_values(dibs_engine* e, bool exported) {
  if (!exported) {
    HIP_OK(hipMemcpy2DAsync(e->vsend, (size_t)e->Ev * 4, e->z, (size_t)e->D * 4, (size_t)e->D * 4, (size_t)e->Mloc, hipMemcpyDeviceToDevice, e->stream));
    if (e->P)
      HIP_OK(hipMemcpy2DAsync(e->vsend + e->D, (size_t)e->Ev * 4, e->theta, (size_t)e->P * 4, (size_t)e->P * 4, (size_t)e->Mloc,
                              hipMemcpyDeviceToDevice, e->stream));
  }
  HIP_OK(hipEventRecord(e->ev_exported, e->stream));
  HIP_OK(hipStreamWaitEvent(e->side, e->ev_exported, 0));
  const float* plane0 = e->planes;
  if (e->ipc.on) {  // value exchange n goes to plane set n & 1 of every arena (the own one included); the gradient rows of that step follow it there
    e->ipc.vset = (int)((e->ipc.seq[1] + 1u) & 1u);
    if (ipc_all_gather(e, 1, e->side, e->vsend, e->ipc.set_off(e->ipc.vset) + (size_t)e->m0 * e->Ev * 4, (size_t)e->Mloc * e->Ev, true)) return 1;
    plane0 = e->ipc.set(e->ipc.vset);
  } else if (e->loopback) {  // (own rows only; a kernel of our own, not hipMemcpyAsync: see k_copy_rows)
    const size_t n4 = (size_t)e->Mloc * e->Ev / 4;  // (Ev is a multiple of 4)
    hipLaunchKernelGGL(k_copy_rows, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, e->side, reinterpret_cast<const float4*>(e->vsend),
                       reinterpret_cast<float4*>(e->planes + (size_t)e->m0 * e->Ev), n4);
  }
  else
    RCCL_OK(rccl().all_gather(e->vsend, e->planes, (size_t)e->Mloc * e->Ev, ncclFloat, e->comm[1], e->side));
  if (dibs_engine_kmat_values(e, plane0, e->side)) return 1;
  HIP_OK(hipEventRecord(e->ev_vals, e->side));
  e->vals_fresh = true;
  return 0;
}

// after the streams have been synchronised: did a rank give up waiting for its peers' rows?
static int ipc_check(dibs_engine* e) {
  if (e->ipc.err && *e->ipc.err) {
    *e->ipc.err = 0u;
    return fail("mapped-memory exchange: the rows of a peer rank did not arrive within the time-out (a rank that died, or ranks that did not "
                "call the same sequence of runs); the results of this chunk are invalid");
  }
  return 0;
}

// the steps of one sharded chunk, enqueued and synchronised
static int run_sharded_steps(dibs_engine* e, int t_start, int n_steps, int overlapped) {
  const size_t grad_plane = (size_t)e->M * e->Ev;
  if (overlapped && !e->vals_fresh && exchange_values(e, false)) return 1;
  for (int t = t_start; t < t_start + n_steps; ++t) {
    if (!overlapped) {
      const int pp = (int)(e->ipc.pack_seq & 1u);
      float* const pk = e->ipc.on ? e->ipc.pack(pp) : e->pack;
      if (step_local(e, t, packed_rows(e, pk))) return 1;
      if (e->ipc.on) {
        if (ipc_all_gather(e, 0, e->stream, pk + (size_t)e->m0 * e->E, e->ipc.pack_off(pp) + (size_t)e->m0 * e->E * 4, (size_t)e->Mloc * e->E, false)) return 1;
        ++e->ipc.pack_seq;
      } else if (!e->loopback)
        RCCL_OK(rccl().all_gather(pk + (size_t)e->m0 * e->E, pk, (size_t)e->Mloc * e->E, ncclFloat, e->comm[0], e->stream));
      if (step_update(e, t, packed_source(e, pk))) return 1;
    } else {
      float* const planes = e->ipc.on ? e->ipc.set(e->ipc.vset) : e->planes;  // (the set the values of this step were gathered into)
      float* const gplane = planes + grad_plane;  // rows [grad_z | grad_theta], indexed by global particle id
      if (step_local(e, t, RowTarget{gplane, (size_t)e->Ev, 0, 0, (size_t)e->D, 0})) return 1;
      if (e->ipc.on) {
        if (ipc_all_gather(e, 0, e->stream, gplane + (size_t)e->m0 * e->Ev, e->ipc.set_off(e->ipc.vset) + (grad_plane + (size_t)e->m0 * e->Ev) * 4,
                           (size_t)e->Mloc * e->Ev, false))
          return 1;
      } else if (!e->loopback)
        RCCL_OK(rccl().all_gather(gplane + (size_t)e->m0 * e->Ev, gplane, (size_t)e->Mloc * e->Ev, ncclFloat, e->comm[0], e->stream));
      HIP_OK(hipStreamWaitEvent(e->stream, e->ev_vals, 0));  // values + kernel slab of this step (gathered during the step before)
      if (step_update(e, t, plane_source(e, planes), e->vsend)) return 1;
      if (exchange_values(e, true)) return 1;  // values of step t + 1, beside its phase A
    }
    if (e->profiling && e->pending.size() > 4096) drain_timers(e);
  }
  HIP_OK(hipStreamSynchronize(e->stream));
  if (e->stream2) HIP_OK(hipStreamSynchronize(e->stream2));
  if (overlapped) HIP_OK(hipStreamSynchronize(e->side));
  if (e->profiling) drain_timers(e);
  HIP_OK(hipGetLastError());
  return ipc_check(e);
}

// Every rank learns whether ANY rank's chunk saw a flag time-out (the rows such a rank exchanged were computed from incomplete operands, so
// all ranks' results are invalid together): one all-gather of the ranks' error words, through the same backend as the rows.  *any = the
// largest word.  Costs one tiny collective + a host round trip per CHUNK.
static int agree_on_error(dibs_engine* e, unsigned int mine, unsigned int* any) {
  *any = mine;
  if (e->loopback || e->cfg.n_ranks == 1) return 0;
  const int R = e->cfg.n_ranks;
  for (int i = 0; i < 4; ++i) e->agree_host[i] = mine;
  HIP_OK(hipMemcpyAsync(e->agree_dev, e->agree_host, 16, hipMemcpyHostToDevice, e->stream));
  if (e->ipc.on) {
    const size_t off = IPC_AGREE_OFF + (size_t)(e->ipc.agree_seq & 1u) * IPC_MAX_RANKS * 16;
    ++e->ipc.agree_seq;
    if (ipc_all_gather(e, 0, e->stream, reinterpret_cast<const float*>(e->agree_dev), off + (size_t)e->cfg.rank * 16, 4, true)) return 1;
    HIP_OK(hipMemcpyAsync(e->agree_host + 4, e->ipc.arena + off, (size_t)R * 16, hipMemcpyDeviceToHost, e->stream));
  } else {
    RCCL_OK(rccl().all_gather(e->agree_dev, e->agree_dev + 4, 4, ncclUint32, e->comm[0], e->stream));
    HIP_OK(hipMemcpyAsync(e->agree_host + 4, e->agree_dev + 4, (size_t)R * 16, hipMemcpyDeviceToHost, e->stream));
  }
  HIP_OK(hipStreamSynchronize(e->stream));
  if (ipc_check(e)) return 1;
  for (int r = 0; r < R; ++r)
    if (e->agree_host[4 + 4 * r] > *any) *any = e->agree_host[4 + 4 * r];
  return 0;
}

// replaces _svgd_loop for a particle-sharded run: every rank calls it with the same (t_start, n_steps).  overlapped = 0: phase A -> ONE
// all-gather of the packed rows [z | grad_z | theta | grad_theta] (in place in the row buffer, on the engine stream) -> phase B.
// overlapped = 1: values gathered on the side stream beside phase A, only the gradient rows between the phases.
// A flag time-out on ANY rank (see latch_flags) makes ALL ranks repeat the chunk on events from their chunk-start copies of the carry.
extern "C" int dibs_engine_run_sharded(dibs_engine* e, int32_t t_start, int32_t n_steps, int32_t overlapped) {
  if (!e) return fail("null engine");
  if (e->f64) return fail("float64 engine: dibs_engine_run_sharded is not supported (dibs_engine_run only)");
  if (refuse_chains(e, "the sharded entry points (chains are not sharded over ranks)")) return 1;
  if (e->B > 1) return fail("batched engine: a batch is not sharded over ranks");
  if (!e->has_data) return fail("dibs_engine_set_data has not been called");
  if (need_edge_prior(e)) return 1;
  if (e->n_comms < 1) return fail("dibs_engine_comm_init has not been called");
  if (overlapped && e->n_comms < 2) return fail("the overlapped exchange needs two communicators (dibs_engine_comm_init with n_ids = 2)");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  latch_flags(e);
  if (n_steps > 0 && carry_copy(e, false)) return 1;
  if (run_sharded_steps(e, t_start, n_steps, overlapped)) return 1;
  if (n_steps <= 0) return 0;
  unsigned int any = 0u;
  if (agree_on_error(e, take_join_err(e), &any)) return 1;
  if (any) {
    e->flags_off = true;
    ++e->flag_fallbacks;
    latch_flags(e);
    if (carry_copy(e, true)) return 1;
    e->vals_fresh = false;  // (the overlapped protocol gathers the restored values again: every rank does)
    if (run_sharded_steps(e, t_start, n_steps, overlapped)) return 1;
    if (agree_on_error(e, take_join_err(e), &any)) return 1;
    if (any) return join_failure(any, " on a rank of this run, twice; the results of this chunk are invalid");
  }
  return 0;
}

// z (and theta) of ALL ranks' particles after a sharded run, on every rank: [M][d][k][2] and [M][P] host buffers (either may be NULL).
// overlapped runs already hold them in plane 0; otherwise one all-gather of the values.
extern "C" int dibs_engine_gather_particles(dibs_engine* e, float* z_all, float* theta_all) {
  if (!e) return fail("null engine");
  if (e->f64) return fail("float64 engine: dibs_engine_gather_particles is not supported (dibs_engine_run only)");
  if (e->n_comms < 1) return fail("dibs_engine_comm_init has not been called");
  if (e->loopback) return fail("loopback communicator (timing only): there are no other ranks to gather from");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  DevBuf<float> tmp_all, tmp_send;
  const float* vals = nullptr;
  if (e->n_comms == 2) {
    if (!e->vals_fresh && exchange_values(e, false)) return 1;
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipStreamSynchronize(e->side));
    if (ipc_check(e)) return 1;
    vals = e->ipc.on ? e->ipc.set(e->ipc.vset) : e->planes;
  } else {
    HIP_OK(tmp_all.alloc((size_t)e->M * e->Ev));
    HIP_OK(tmp_send.alloc((size_t)e->Mloc * e->Ev));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy2DAsync(tmp_send.p, (size_t)e->Ev * 4, e->z, (size_t)e->D * 4, (size_t)e->D * 4, (size_t)e->Mloc, hipMemcpyDeviceToDevice, e->stream));
    if (e->P)
      HIP_OK(hipMemcpy2DAsync(tmp_send.p + e->D, (size_t)e->Ev * 4, e->theta, (size_t)e->P * 4, (size_t)e->P * 4, (size_t)e->Mloc,
                              hipMemcpyDeviceToDevice, e->stream));
    RCCL_OK(rccl().all_gather(tmp_send.p, tmp_all.p, (size_t)e->Mloc * e->Ev, ncclFloat, e->comm[0], e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    vals = tmp_all.p;
  }
  if (z_all) HIP_OK(hipMemcpy2D(z_all, (size_t)e->D * 4, vals, (size_t)e->Ev * 4, (size_t)e->D * 4, (size_t)e->M, hipMemcpyDeviceToHost));
  if (theta_all && e->P)
    HIP_OK(hipMemcpy2D(theta_all, (size_t)e->P * 4, vals + e->D, (size_t)e->Ev * 4, (size_t)e->P * 4, (size_t)e->M, hipMemcpyDeviceToHost));
  return 0;
}
