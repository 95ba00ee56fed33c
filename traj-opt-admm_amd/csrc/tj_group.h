// tj_group.h -- several GPUs under ONE host process, inside the library.  Included at the end of tj_api.hip.
//
// The reference is single-process, single-thread; its per-robot loops (Optimization3D_multi.h:29-118) are what shards.  A group
// is one sharded context per rank (robots block-partitioned exactly like tj_params.rank/world), each on its own device and
// stream, driven by one host thread per rank so that the enqueue cost (~3.5 us per launch) does not add up over the ranks.  An
// iteration is the same phase list tj_iterate_phase exposes; after a phase that produces something every rank needs
// (tj_exchange_buffer: control points, direction records, and in coupled mode the Schur-corner terms, CCD exponents and
// Armijo energies) the slices are exchanged by one of three TRANSPORTS (TJ_GROUP_TRANSPORT=flag|event|rccl, or
// tj_group_set_transport):
//
//   flag   (opt-in until it has run across xGMI; the fastest with ranks on one device) device-to-device, no host on the path, no event, no collective
//          library.  k_group_push: the owner stores its slice straight into a receive buffer on EVERY peer (peer-mapped memory:
//          N-1 point-to-point xGMI transfers leave in parallel, there is no ring), fences at system scope and then stores the
//          exchange's sequence number into its flag word on every peer.  k_group_wait_unpack, next on the consumer's own stream:
//          one lane per peer polls that peer's flag word (system-scope acquire; wall-clock timeout -> ERR_PEER_TIMEOUT, never a
//          hang), then the block moves the foreign slices into the buffer the kernels read.  Two small launches per exchange.
//   event  (the default: plain HIP stream / event semantics; ranks sharing a GPU may share a hardware queue, where the flag
//          transport's polling kernel could sit in front of the very push it waits for) k_group_push, hipEventRecord; the peers' host threads wait for the record to
//          exist and make their streams wait on the event (hipStreamWaitEvent), then k_group_unpack.
//   rccl   the collective north_star names, driven from host C++: ncclCommInitAll over the group's devices, one in-place
//          ncclAllGather per exchange on each rank's solver stream (called by that rank's host thread).  librccl.so is opened
//          at run time (dlopen) only when this transport is asked for -- the library has no link-time dependency on it.
//          Needs distinct devices and U divisible by the number of ranks (equal slices); refused otherwise.
//
// Receive buffers and flag words are UNCACHED device memory (hipExtMallocWithFlags(hipDeviceMallocUncached)): they are
// written by a remote GPU and read by a later local kernel, and the same-parity buffer was read two exchanges earlier, so
// ordinary cached memory could serve stale lines; the events of the event transport release to system scope.  Buffers are
// double-buffered by exchange parity: a peer can run at most one exchange of the same kind ahead, because its next push
// follows its own wait on everybody's current one.  The payload is <= 30 KB per rank, so the exchange is latency, not
// bandwidth.  Results are bitwise those of one context (tests run ranks on the same device, which the design allows: `devices`
// may repeat).  A group whose devices are all distinct has NOT run on hardware yet (no multi-GPU box was available in rounds
// 1-3): tests/test_gpu_group.py::test_group_on_two_devices runs wherever two devices are visible.
#pragma once
#include <algorithm>
#include <atomic>
#include <mutex>
#include <thread>
#include <dlfcn.h>

namespace tj {

constexpr int GROUP_MAX = 16;
struct GroupPeers { double* p[GROUP_MAX]; unsigned long long* flag[GROUP_MAX]; };

__global__ __launch_bounds__(256) void k_group_push(const double* src, GroupPeers dst, int n_peers, size_t off, size_t count) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    const double v = src[off + i];
    for (int q = 0; q < n_peers; q++) dst.p[q][off + i] = v;
  }
}
// everything outside [own_off, own_off + own_count) of a buffer of `total` doubles
__global__ __launch_bounds__(256) void k_group_unpack(double* dst, const double* rx, size_t own_off, size_t own_count, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    if (i < own_off || i >= own_off + own_count) dst[i] = rx[i];
}

// flag transport.  ONE block: its barrier is what orders "every thread's stores are fenced" before the flags go out.
constexpr int GROUP_FLAG_THREADS = 1024;
__global__ __launch_bounds__(GROUP_FLAG_THREADS) void k_group_push_flag(const double* src, GroupPeers dst, int n_peers, size_t off, size_t count, unsigned long long seq) {
  for (size_t i = threadIdx.x; i < count; i += GROUP_FLAG_THREADS) {
    const double v = src[off + i];
    for (int q = 0; q < n_peers; q++) dst.p[q][off + i] = v;
  }
  __threadfence_system();
  __syncthreads();
  if ((int)threadIdx.x < n_peers) __hip_atomic_store(dst.flag[threadIdx.x], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// flags: this rank's words, one per peer (already offset to the exchange's kind and parity).  Wave 0 waits for every peer's flag (lane p: peer p), the block behind it.
__global__ __launch_bounds__(GROUP_FLAG_THREADS) void k_group_wait_unpack(double* dst, const double* rx, GroupPeers mine, int n_peers, unsigned long long seq, size_t own_off, size_t own_count, size_t total, Ctl* ctl) {
  __shared__ int s_lost;
  if (threadIdx.x < 64) {
    const unsigned long long* f = (int)threadIdx.x < n_peers ? mine.flag[threadIdx.x] : nullptr;
    const bool ok = poll_until<8>([&] { return ballot(f && __hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < seq) == 0ull; }, WAIT_2S);
    if (threadIdx.x == 0) { s_lost = !ok; if (!ok) atomicOr(&ctl->error, ERR_PEER_TIMEOUT); }
  }
  __syncthreads();
  if (s_lost) return;   // a peer's slice never arrived: leave the buffer as it is (the error bit fails the batch) rather than unpack stale data
  for (size_t i = threadIdx.x; i < total; i += GROUP_FLAG_THREADS)
    if (i < own_off || i >= own_off + own_count) dst[i] = __builtin_nontemporal_load(rx + i);
}

}  // namespace tj

// ---- RCCL, resolved at run time ---------------------------------------------------------------------------------------------
namespace {
struct RcclApi {
  void* lib = nullptr;
  int (*CommInitAll)(void** comms, int ndev, const int* devlist) = nullptr;                                         // ncclCommInitAll
  int (*CommDestroy)(void* comm) = nullptr;                                                                          // ncclCommDestroy
  int (*AllGather)(const void* send, void* recv, size_t count, int dtype, void* comm, hipStream_t stream) = nullptr;  // ncclAllGather
  const char* (*GetErrorString)(int) = nullptr;                                                                      // ncclGetErrorString
  int (*CommCount)(void* comm, int* count) = nullptr;                                                                // ncclCommCount (optional: reporting only)
  int (*Broadcast)(const void* send, void* recv, size_t count, int dtype, int root, void* comm, hipStream_t stream) = nullptr;   // ncclBroadcast  } optional: unequal slices
  int (*GroupStart)() = nullptr; int (*GroupEnd)() = nullptr;                                                        // ncclGroupStart / ncclGroupEnd  } (uav_num % ranks != 0)
  bool uneven_ok() const { return Broadcast && GroupStart && GroupEnd; }
  std::string err;                                                                                                   // why the library could not be bound (taken once, where dlopen failed)
  bool ok() const { return lib && CommInitAll && CommDestroy && AllGather && GetErrorString; }
};
constexpr int kNcclFloat64 = 8;   // ncclDouble / ncclFloat64 (rccl.h ncclDataType_t)
RcclApi& rccl_api() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
      api.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
      if (api.lib) break;
      const char* e = dlerror();   // one call: dlerror() clears the pending message
      if (!api.err.empty()) api.err += "; ";
      api.err += e ? e : (std::string(n) + ": dlopen failed");
    }
    if (!api.lib) return;
    api.err.clear();
    api.CommInitAll = (decltype(api.CommInitAll))dlsym(api.lib, "ncclCommInitAll");
    api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.lib, "ncclCommDestroy");
    api.AllGather = (decltype(api.AllGather))dlsym(api.lib, "ncclAllGather");
    api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.lib, "ncclGetErrorString");
    api.CommCount = (decltype(api.CommCount))dlsym(api.lib, "ncclCommCount");
    api.Broadcast = (decltype(api.Broadcast))dlsym(api.lib, "ncclBroadcast");
    api.GroupStart = (decltype(api.GroupStart))dlsym(api.lib, "ncclGroupStart");
    api.GroupEnd = (decltype(api.GroupEnd))dlsym(api.lib, "ncclGroupEnd");
    if (!api.ok()) api.err = "librccl.so lacks ncclCommInitAll / ncclCommDestroy / ncclAllGather / ncclGetErrorString";
  });
  return api;
}
}  // namespace

enum { TJ_TRANSPORT_EVENT = 0, TJ_TRANSPORT_FLAG = 1, TJ_TRANSPORT_RCCL = 2 };

struct tj_group {
  int n = 0;
  int lsc_followed = 0;                           // coupled mode: batches that were run again with the Armijo search followed beyond the exchanged candidates (tj_group_iterate)
  int transport = TJ_TRANSPORT_EVENT;
  bool distinct = false;                          // every rank on its own device
  std::vector<tj_ctx*> ctx;
  std::vector<int> dev;
  double* rx[tj::GROUP_MAX][5][2] = {};           // uncached receive buffers
  unsigned long long* flags[tj::GROUP_MAX] = {};  // uncached [5][2][GROUP_MAX]: sequence number of the last push of (what, parity) by each peer
  hipEvent_t ev[tj::GROUP_MAX][5][2] = {};
  std::atomic<long> recorded[tj::GROUP_MAX][5];   // pushes of buffer `what` rank r has recorded so far (event transport)
  long issued[5] = {0, 0, 0, 0, 0};               // exchanges of each kind completed by earlier tj_group_iterate calls
  std::atomic<int> abort_flag{0};
  bool poisoned = false;                          // a rank failed mid-batch: the ranks' exchange counts no longer agree
  std::vector<void*> comms;                       // ncclComm_t per rank (rccl transport)
  std::vector<void*> uncached;                    // hipExtMallocWithFlags allocations, with their device
  std::vector<int> uncached_dev;
  std::string err;
};

namespace {

struct GroupExchangeInfo { double* buf; size_t per; };
GroupExchangeInfo group_buffer(tj_ctx* c, int what) {
  void* p = nullptr; int per = 0;
  tj_exchange_buffer(c, what, &p, &per, nullptr, nullptr);
  return {(double*)p, (size_t)per};
}
inline unsigned long long* group_flag(tj_group* g, int rank, int what, int par, int src) { return g->flags[rank] + ((size_t)(what * 2 + par) * tj::GROUP_MAX + src); }

// one exchange of buffer `what`, issued by rank r's host thread; s = how many exchanges of this kind came before
int group_exchange(tj_group* g, int r, int what, long s) {
  tj_ctx* c = g->ctx[r];
  const Dev& d = c->d;
  if (g->n == 1) return TJ_OK;   // nothing is foreign
  const int par = (int)(s & 1);
  const GroupExchangeInfo b = group_buffer(c, what);
  const size_t off = (size_t)d.u0 * b.per, cnt = (size_t)(d.u1 - d.u0) * b.per, total = (size_t)d.U * b.per;
  if (g->transport == TJ_TRANSPORT_RCCL) {   // in place: this rank's slice already sits at its offset of the full buffer
    RcclApi& api = rccl_api();
    c->launches++;   // (the collective's kernel)
    if (d.U % g->n == 0) {
      const int rc = api.AllGather(b.buf + off, b.buf, cnt, kNcclFloat64, g->comms[r], c->stream);
      if (rc != 0) { c->err = std::string("ncclAllGather: ") + api.GetErrorString(rc); return TJ_ERR_DEVICE; }
      return TJ_OK;
    }
    // unequal slices (uav_num not divisible by the ranks): one in-place broadcast per owner, fused into one group call
    int rc = api.GroupStart();
    for (int q = 0; q < g->n && rc == 0; q++) {
      const size_t qo = (size_t)((long long)q * d.U / g->n) * b.per, qc = (size_t)((long long)(q + 1) * d.U / g->n) * b.per - qo;
      if (qc > 0) rc = api.Broadcast(b.buf + qo, b.buf + qo, qc, kNcclFloat64, q, g->comms[r], c->stream);
    }
    const int rc2 = api.GroupEnd();
    if (rc == 0) rc = rc2;
    if (rc != 0) { c->err = std::string("ncclBroadcast (unequal slices): ") + api.GetErrorString(rc); return TJ_ERR_DEVICE; }
    return TJ_OK;
  }
  GroupPeers peers; int np = 0;
  for (int q = 0; q < g->n; q++) if (q != r) { peers.p[np] = g->rx[q][what][par]; peers.flag[np] = group_flag(g, q, what, par, r); np++; }
  if (g->transport == TJ_TRANSPORT_FLAG) {
    GroupPeers mine; int nm = 0;
    for (int q = 0; q < g->n; q++) if (q != r) { mine.p[nm] = nullptr; mine.flag[nm] = group_flag(g, r, what, par, q); nm++; }
    TJ_LAUNCH(k_group_push_flag, dim3(1), dim3(GROUP_FLAG_THREADS), 0, c->stream, b.buf, peers, np, off, cnt, (unsigned long long)(s + 1));
    TJ_LAUNCH(k_group_wait_unpack, dim3(1), dim3(GROUP_FLAG_THREADS), 0, c->stream, b.buf, g->rx[r][what][par], mine, nm, (unsigned long long)(s + 1), off, cnt, total, d.ctl);
    HIPCHK(c, hipGetLastError());
    return TJ_OK;
  }
  const bool direct = d.xch != 0;   // decoupled mode: the producing kernel itself has stored this rank's slice into the peers' receive blocks (kernels_step.h) -- the event
                                    // only orders the consumer's stream behind it, and the foreign units of its next kernel put the slices in place
  if (cnt > 0 && !direct) TJ_LAUNCH(k_group_push, dim3((unsigned)std::min<size_t>((cnt + 255) / 256, 64)), dim3(256), 0, c->stream, b.buf, peers, np, off, cnt);
  HIPCHK(c, hipEventRecord(g->ev[r][what][par], c->stream));
  g->recorded[r][what].store(s + 1, std::memory_order_release);
  for (int q = 0; q < g->n; q++) {
    if (q == r) continue;
    while (g->recorded[q][what].load(std::memory_order_acquire) < s + 1) {   // the peer's host thread has not recorded this push yet
      if (g->abort_flag.load(std::memory_order_relaxed)) { c->err = "group: a peer rank failed"; return TJ_ERR_DEVICE; }
      std::this_thread::yield();
    }
    HIPCHK(c, hipStreamWaitEvent(c->stream, g->ev[q][what][par], 0));
  }
  if (!direct) TJ_LAUNCH(k_group_unpack, dim3((unsigned)std::min<size_t>((total + 255) / 256, 64)), dim3(256), 0, c->stream, b.buf, g->rx[r][what][par], off, cnt, total);
  HIPCHK(c, hipGetLastError());
  return TJ_OK;
}

// (phase, buffer exchanged after it or -1): the schedules of traj-opt-admm_amd/sharding.py
const int kGroupDecoupled[][2] = {{0, 0}, {1, 1}, {2, -1}};
const int kGroupCoupled[][2] = {{0, 0}, {1, 2}, {2, 1}, {3, 3}, {4, 4}, {5, -1}};

// careful (coupled mode, the re-run of a batch whose Armijo search left the candidates one exchange carries): the rank follows the search -- after phase 5 it asks
// tj_coupled_search_pending (one host look per iteration) and repeats phase 4 / exchange 4 / phase 5 while the answer is yes; *extra4 = the additional exchanges of
// buffer 4 it issued (the same number on every rank: same gathered tables, same decisions)
int group_rank_loop(tj_group* g, int r, int n_iters, bool careful = false, long* extra4 = nullptr) {
  tj_ctx* c = g->ctx[r];
  HIPCHK(c, hipSetDevice(g->dev[r]));
  if (!ready(c)) return TJ_ERR_INVALID;
  const bool cpl = c->d.mode == TJ_MODE_MULTI_COUPLED;
  const int (*sched)[2] = cpl ? kGroupCoupled : kGroupDecoupled;
  const int nph = cpl ? 6 : 3;
  // direct exchange (flag transport, decoupled mode): nothing between the launches -- the producing kernels push, the consuming kernels wait:
  // the fused six-kernel chain of one context
  if (g->n > 1 && g->transport == TJ_TRANSPORT_FLAG && c->d.xch) return tj_iterate_async(c, n_iters);
  long s[5];
  for (int w = 0; w < 5; w++) s[w] = g->issued[w];
  for (int it = 0; it < n_iters; it++) {
    for (int k = 0; k < nph; k++) {
      int rc = tj_iterate_phase_chained(c, sched[k][0], it + 1 < n_iters);   // (decoupled: the next iteration's begin rides in this one's k_linesearch)
      if (rc) return rc;
      const int what = sched[k][1];
      if (what >= 0) { rc = group_exchange(g, r, what, s[what]++); if (rc) return rc; }
    }
    if (careful && cpl)
      for (;;) {
        int pending = 0;
        int rc = tj_coupled_search_pending(c, &pending); if (rc) return rc;
        if (!pending) break;
        if ((rc = tj_iterate_phase_chained(c, 4, 0)) || (rc = group_exchange(g, r, 4, s[4]++)) || (rc = tj_iterate_phase_chained(c, 5, 0))) return rc;
        if (extra4) (*extra4)++;
      }
  }
  return TJ_OK;
}

// Direct exchange, ranks that share a device: HIP maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues per device and lets further streams share them, and a
// shared queue starts its kernels one after another in submission order.  A kernel that waits for a peer's push must then never be submitted ahead of the kernel that
// pushes: with three ranks on a device of two queues a rank's k_front / k_ccd waited at the head of a queue for a peer whose producer stood behind it, until the 2 s limit.
// So one host thread enqueues the batch for all ranks, iteration by iteration and part by part, every rank's part before any rank's next part: k_begin (pushes the
// control points at a batch's start), k_hullinfo .. k_xsolve (k_front waits for the control points, k_xsolve pushes the direction records), k_ccd .. k_linesearch (k_ccd
// waits for the direction records, k_linesearch pushes the control points of the next iteration) -- every wait stands behind its producers in whatever queue they share.
// Same kernels and chain positions per rank as tj_iterate_async; only the host's interleaving differs.
int group_direct_lockstep(tj_group* g, int n_iters, std::vector<int>& rc) {
  for (int r = 0; r < g->n; r++) {
    tj_ctx* c = g->ctx[r];
    if (hipSetDevice(g->dev[r]) != hipSuccess) { c->err = "hipSetDevice failed"; return rc[r] = TJ_ERR_DEVICE; }
    if (!ready(c)) return rc[r] = TJ_ERR_INVALID;
    if ((rc[r] = iterate_async_prologue(c, n_iters))) return rc[r];
  }
  for (int i = 0; i < n_iters; i++) {
    std::vector<int> pos(g->n);
    static const int cut[4] = {0, K_HULLINFO, K_CCD_PREP, K_COUNT};
    for (int part = 0; part < 3; part++)
      for (int r = 0; r < g->n; r++) {
        tj_ctx* c = g->ctx[r];
        if (hipSetDevice(g->dev[r]) != hipSuccess) { c->err = "hipSetDevice failed"; return rc[r] = TJ_ERR_DEVICE; }
        if (part == 0) pos[r] = iterate_async_pos(c, i, n_iters);
        if ((rc[r] = enqueue_iteration(c, pos[r], cut[part], cut[part + 1]))) return rc[r];
      }
  }
  return TJ_OK;
}

int group_fail(tj_group* g, int rc, const std::string& m) { g->err = m; return rc; }
thread_local std::string g_group_create_err;   // why this thread's last tj_group_create failed (there is no group to ask then)

const char* transport_name(int t) { return t == TJ_TRANSPORT_FLAG ? "flag" : (t == TJ_TRANSPORT_RCCL ? "rccl" : "event"); }

// (re)select the transport; rccl communicators are created on first selection
int group_select_transport(tj_group* g, int t) {
  if (t == TJ_TRANSPORT_RCCL) {
    if (!g->distinct) return group_fail(g, TJ_ERR_UNSUPPORTED, "transport rccl needs every rank on its own device (RCCL refuses two ranks on one GPU)");
    RcclApi& api = rccl_api();
    if (!api.ok()) return group_fail(g, TJ_ERR_DEVICE, std::string("transport rccl: librccl.so could not be bound: ") + (api.err.empty() ? std::string("symbols missing") : api.err));
    if (g->ctx[0]->d.U % g->n != 0 && !api.uneven_ok()) return group_fail(g, TJ_ERR_UNSUPPORTED, "transport rccl: the robot count is not divisible by the number of ranks and this librccl.so lacks ncclBroadcast / ncclGroupStart / ncclGroupEnd (unequal slices go out as one grouped broadcast per owner)");
    if (g->comms.empty()) {
      g->comms.assign(g->n, nullptr);
      const int rc = api.CommInitAll(g->comms.data(), g->n, g->dev.data());
      if (rc != 0) { g->comms.clear(); return group_fail(g, TJ_ERR_DEVICE, std::string("ncclCommInitAll: ") + api.GetErrorString(rc)); }
    }
  }
  // flag transport, decoupled mode: the DIRECT exchange (in-kernel pushes and waits, csrc/kernels_step.h).  Ranks that share a device do not poll inside
  // k_front / k_ccd (their waiting waves would hold the LDS the peer's producing kernel needs): a one-wave wait launch in front instead.
  // TJ_XCH_POLL=1 / 0 overrides (test hook: small fleets can poll on a shared device).
  for (int r = 0; r < g->n; r++) {
    tj_ctx* c = g->ctx[r];
    if (!c->d.xf || !c->d.xp) continue;
    (void)hipSetDevice(g->dev[r]);
    int sharers = 0;
    for (int b = 0; b < g->n; b++) sharers += g->dev[b] == g->dev[r] ? 1 : 0;
    // ranks sharing a device: k_linesearch's helper blocks (one compute unit each) only where the ranks run in lockstep (flag: the kernels of the ranks overlap and every
    // helper is resident; measured with 2 x 32 robots on one device: 0.147 -> 0.137 ms) -- under the event transport, which orders whole kernels, the helpers of one rank
    // queue behind the other rank's blocks and the primaries run into their 10 us give-up (0.166 -> 0.279 ms)
    if (sharers > 1 && !c->hp.ls_help_forced && c->d.ls_fast && c->d.mode != TJ_MODE_MULTI_COUPLED)
      c->d.ls_help = t == TJ_TRANSPORT_FLAG ? plan_ls_help(c->d, c->hp, c->d.num_cu / sharers) : 1;   // (the planner's rule on this rank's share of the compute units)
    int wait_mode = sharers == 1 ? 1 : 0;
    if (const char* e = tune("XCH_POLL")) wait_mode = atoi(e) != 0 ? 1 : 0;
    if (t == TJ_TRANSPORT_EVENT) wait_mode = 2;   // events order the streams
    const int rc = tj_xch_enable(c, t != TJ_TRANSPORT_RCCL ? 1 : 0, wait_mode);
    if (rc) return group_fail(g, rc, std::string("rank ") + std::to_string(r) + ": " + tj_last_error(c));
  }
  g->transport = t;
  return TJ_OK;
}

}  // namespace

extern "C" {

int tj_rccl_available(void) { return rccl_api().ok() ? 1 : 0; }   // librccl.so opens and exports the four entry points the rccl transport binds (no GPU needed)

int tj_group_create(const tj_params* p, int n_ranks, const int* devices, tj_group** out) {
  if (!p || !out || n_ranks < 1 || n_ranks > tj::GROUP_MAX) return TJ_ERR_INVALID;
  if (p->mode == TJ_MODE_SINGLE && n_ranks > 1) return TJ_ERR_INVALID;   // one robot does not shard
  tj_group* g = new tj_group();
  g->n = n_ranks;
  for (int r = 0; r < n_ranks; r++) for (int w = 0; w < 5; w++) g->recorded[r][w].store(0);
  auto bail = [&](int rc, const std::string& m) { g_group_create_err = m; tj_group_destroy(g); return rc; };
  for (int r = 0; r < n_ranks; r++) g->dev.push_back(devices ? devices[r] : r);
  g->distinct = true;
  for (int a = 0; a < n_ranks; a++) for (int b = a + 1; b < n_ranks; b++) if (g->dev[a] == g->dev[b]) g->distinct = false;
  // peers write into each other's receive buffers
  for (int a = 0; a < n_ranks; a++) for (int b = 0; b < n_ranks; b++) {
    if (g->dev[a] == g->dev[b]) continue;
    int can = 0;
    if (hipSetDevice(g->dev[a]) != hipSuccess || hipDeviceCanAccessPeer(&can, g->dev[a], g->dev[b]) != hipSuccess || !can) return bail(TJ_ERR_UNSUPPORTED, "no peer access between the devices of the group");
    hipError_t e = hipDeviceEnablePeerAccess(g->dev[b], 0);
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return bail(TJ_ERR_DEVICE, "hipDeviceEnablePeerAccess failed");
    (void)hipGetLastError();
  }
  auto ualloc = [&](int dev, size_t bytes, void** out_p) -> bool {   // uncached device memory, zeroed
    if (hipSetDevice(dev) != hipSuccess) return false;
    void* q = nullptr;
    if (hipExtMallocWithFlags(&q, std::max<size_t>(bytes, 8), hipDeviceMallocUncached) != hipSuccess) { (void)hipGetLastError(); return false; }
    g->uncached.push_back(q); g->uncached_dev.push_back(dev);
    if (hipMemset(q, 0, std::max<size_t>(bytes, 8)) != hipSuccess) return false;
    *out_p = q;
    return true;
  };
  for (int r = 0; r < n_ranks; r++) {
    tj_params q = *p;
    q.rank = r; q.world = n_ranks; q.device = g->dev[r];
    tj_ctx* c = nullptr;
    const int rc = tj_create(&q, &c);
    if (rc) { const std::string m = std::string("rank ") + std::to_string(r) + ": " + tj_last_error(c); if (c) tj_destroy(c); return bail(rc, m); }
    g->ctx.push_back(c);
    {   // ranks that share a device (a test arrangement) share its compute units too: k_linesearch's helper blocks (one CU each) and k_grad's launch order assume
        // a device of their own -- off for those ranks (same bits either way)
      int sharers = 0;
      for (int b = 0; b < n_ranks; b++) sharers += g->dev[b] == g->dev[r] ? 1 : 0;
      if (sharers > 1) { c->d.ls_help = 1; c->d.grad_bal = 0; c->hp.lsc_wide = false; }   // (ls_help: re-decided per transport, group_select_transport)
    }
    const int nwhat = c->d.mode == TJ_MODE_MULTI_COUPLED ? 5 : 2;
    for (int w = 0; w < nwhat; w++) {
      const GroupExchangeInfo b = group_buffer(c, w);
      for (int par = 0; par < 2; par++) {
        if (!ualloc(g->dev[r], (size_t)c->d.U * b.per * sizeof(double), (void**)&g->rx[r][w][par])) return bail(TJ_ERR_DEVICE, "receive buffer allocation failed (hipExtMallocWithFlags, uncached)");
        if (hipEventCreateWithFlags(&g->ev[r][w][par], hipEventDisableTiming | hipEventReleaseToSystem) != hipSuccess) return bail(TJ_ERR_DEVICE, "hipEventCreate failed");
      }
    }
    if (!ualloc(g->dev[r], sizeof(unsigned long long) * 5 * 2 * tj::GROUP_MAX, (void**)&g->flags[r])) return bail(TJ_ERR_DEVICE, "flag allocation failed (hipExtMallocWithFlags, uncached)");
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return bail(TJ_ERR_DEVICE, "stream synchronisation failed");
  }
  // direct exchange (decoupled mode): every rank's receive block, attached to every other rank (peer access is enabled above)
  if (n_ranks > 1 && g->ctx[0]->d.xf) {
    bool ok = true;
    std::vector<void*> base(n_ranks, nullptr);
    for (int r = 0; r < n_ranks && ok; r++) { (void)hipSetDevice(g->dev[r]); ok = tj_xch_block(g->ctx[r], &base[r], nullptr) == TJ_OK; }
    for (int r = 0; r < n_ranks && ok; r++) {
      std::vector<int> pr; std::vector<void*> pb;
      for (int q = 0; q < n_ranks; q++) if (q != r) { pr.push_back(q); pb.push_back(base[q]); }
      (void)hipSetDevice(g->dev[r]);
      ok = tj_xch_attach(g->ctx[r], (int)pr.size(), pr.data(), pb.data()) == TJ_OK;
    }
    // (a group that cannot have it -- more ranks than robots -- keeps the legacy flag kernels; the other transports do not need it)
    if (!ok) for (int r = 0; r < n_ranks; r++) g->ctx[r]->d.xp = nullptr;
  }
  // Default: event, on distinct devices too.  The flag transport (no host, no event on the path) is the fastest one measured with the ranks
  // on one device, but it has not crossed xGMI yet: it is opt-in (TJ_GROUP_TRANSPORT=flag / tj_group_set_transport) until
  // test_group_on_two_devices[flag] has passed on a multi-GPU box; bench.py tries flag -> event -> rccl and validates each bitwise.
  int t = TJ_TRANSPORT_EVENT;
  if (const char* e = tune("GROUP_TRANSPORT")) {
    if (!strcmp(e, "flag")) t = TJ_TRANSPORT_FLAG; else if (!strcmp(e, "event")) t = TJ_TRANSPORT_EVENT; else if (!strcmp(e, "rccl")) t = TJ_TRANSPORT_RCCL;
    else return bail(TJ_ERR_INVALID, std::string("TJ_GROUP_TRANSPORT=") + e + ": expected flag, event or rccl");
  }
  if (n_ranks > 1) { const int rc = group_select_transport(g, t); if (rc) { const std::string m = g->err; return bail(rc, m); } }
  else g->transport = t == TJ_TRANSPORT_RCCL ? TJ_TRANSPORT_EVENT : t;
  *out = g;
  return TJ_OK;
}

void tj_group_destroy(tj_group* g) {
  if (!g) return;
  for (size_t r = 0; r < g->ctx.size(); r++) {
    (void)hipSetDevice(g->dev[r]);
    (void)hipStreamSynchronize(g->ctx[r]->stream);
  }
  for (void* cm : g->comms) if (cm) (void)rccl_api().CommDestroy(cm);
  for (size_t r = 0; r < g->ctx.size(); r++) {
    (void)hipSetDevice(g->dev[r]);
    for (int w = 0; w < 5; w++) for (int par = 0; par < 2; par++) if (g->ev[r][w][par]) (void)hipEventDestroy(g->ev[r][w][par]);
    tj_destroy(g->ctx[r]);
  }
  for (size_t i = 0; i < g->uncached.size(); i++) { (void)hipSetDevice(g->uncached_dev[i]); (void)hipFree(g->uncached[i]); }
  delete g;
}

int tj_group_size(tj_group* g) { return g ? g->n : TJ_ERR_INVALID; }
tj_ctx* tj_group_ctx(tj_group* g, int rank) { return (g && rank >= 0 && rank < g->n) ? g->ctx[rank] : nullptr; }
const char* tj_group_last_error(tj_group* g) { return g ? g->err.c_str() : g_group_create_err.c_str(); }
const char* tj_group_transport(tj_group* g) { return g ? transport_name(g->transport) : ""; }
// ranks the group's RCCL communicator reports (ncclCommCount of rank 0's comm); 0 unless the rccl transport is selected and initialised
int tj_group_rccl_ranks(tj_group* g) {
  if (!g) return TJ_ERR_INVALID;
  if (g->transport != TJ_TRANSPORT_RCCL || g->comms.empty() || !g->comms[0] || !rccl_api().CommCount) return 0;
  int n = 0;
  return rccl_api().CommCount(g->comms[0], &n) == 0 ? n : 0;
}
int tj_group_set_transport(tj_group* g, const char* name) {
  if (!g || !name) return TJ_ERR_INVALID;
  if (g->poisoned) return group_fail(g, TJ_ERR_DEVICE, "group is poisoned by an earlier failure: " + g->err);
  int t;
  if (!strcmp(name, "flag")) t = TJ_TRANSPORT_FLAG; else if (!strcmp(name, "event")) t = TJ_TRANSPORT_EVENT; else if (!strcmp(name, "rccl")) t = TJ_TRANSPORT_RCCL;
  else return group_fail(g, TJ_ERR_INVALID, std::string("unknown transport ") + name);
  // the exchange counters are shared by the transports, but flag words / events of exchanges done under another transport
  // were never written: only switch between batches, and restart the sequence numbers so that parity and flags agree
  for (size_t r = 0; r < g->ctx.size(); r++) { (void)hipSetDevice(g->dev[r]); (void)hipStreamSynchronize(g->ctx[r]->stream); }
  for (int w = 0; w < 5; w++) { g->issued[w] = 0; for (int r = 0; r < g->n; r++) g->recorded[r][w].store(0); }
  for (int r = 0; r < g->n; r++) { (void)hipSetDevice(g->dev[r]); if (g->flags[r]) (void)hipMemset(g->flags[r], 0, sizeof(unsigned long long) * 5 * 2 * tj::GROUP_MAX); (void)hipDeviceSynchronize(); }
  return g->n > 1 ? group_select_transport(g, t) : TJ_OK;
}

#define GROUP_EACH(g, call)                                                                                     \
  for (int r_ = 0; r_ < (g)->n; r_++) {                                                                         \
    tj_ctx* c = (g)->ctx[r_];                                                                                   \
    if (hipSetDevice((g)->dev[r_]) != hipSuccess) return group_fail(g, TJ_ERR_DEVICE, "hipSetDevice failed");   \
    const int rc_ = (call);                                                                                     \
    if (rc_ < 0) return group_fail(g, rc_, std::string("rank ") + std::to_string(r_) + ": " + tj_last_error(c)); \
  }
#define GROUP_LIVE(g) do { if (!(g)) return TJ_ERR_INVALID; if ((g)->poisoned) return TJ_ERR_DEVICE; } while (0)   /* the stored error says which rank failed and why */

int tj_group_set_cloud(tj_group* g, const double* points, int n) { GROUP_LIVE(g); GROUP_EACH(g, tj_set_cloud(c, points, n)); return TJ_OK; }
int tj_group_set_mesh(tj_group* g, const double* verts, int n_verts, const int* tris, int n_tris) { GROUP_LIVE(g); GROUP_EACH(g, tj_set_mesh(c, verts, n_verts, tris, n_tris)); return TJ_OK; }
// also the way out of a poisoned group: every stream is drained, the exchange counters, flag words and recorded counts restart
int tj_group_init_state(tj_group* g, const double* waypoints, double piece_time) {
  if (!g) return TJ_ERR_INVALID;
  for (size_t r = 0; r < g->ctx.size(); r++) { (void)hipSetDevice(g->dev[r]); (void)hipStreamSynchronize(g->ctx[r]->stream); }
  for (int w = 0; w < 5; w++) { g->issued[w] = 0; for (int r = 0; r < g->n; r++) g->recorded[r][w].store(0); }
  for (int r = 0; r < g->n; r++) { (void)hipSetDevice(g->dev[r]); if (g->flags[r]) (void)hipMemset(g->flags[r], 0, sizeof(unsigned long long) * 5 * 2 * tj::GROUP_MAX); (void)hipDeviceSynchronize(); }
  g->poisoned = false;
  GROUP_EACH(g, tj_init_state(c, waypoints, piece_time));   // (also restarts the direct exchange's arrival counters: every stream is drained here)
  return TJ_OK;
}

int tj_group_iterate(tj_group* g, int n_iters, double* gnorm, int* iters_total, int* converged) {
  if (!g || n_iters < 0) return TJ_ERR_INVALID;
  if (g->poisoned) return TJ_ERR_DEVICE;
  g->abort_flag.store(0);
  std::vector<int> rc(g->n, TJ_OK);
  const bool cpl_sharded = g->n > 1 && g->ctx[0]->d.mode == TJ_MODE_MULTI_COUPLED;
  if (cpl_sharded)   // checkpoint of the state the batch starts from: a search that leaves the exchanged candidates (error bit 32) is followed in a second, careful run of the batch (below)
    for (int r = 0; r < g->n; r++) {
      tj_ctx* c = g->ctx[r];
      if (hipSetDevice(g->dev[r]) != hipSuccess) return group_fail(g, TJ_ERR_DEVICE, "hipSetDevice failed");
      int fr = flush_deferred(c);   // (the update the previous batch still owes belongs to the state)
      if (fr || (fr = checkpoint_take(c, false))) return group_fail(g, fr, std::string("rank ") + std::to_string(r) + ": " + tj_last_error(c));
    }
  // direct exchange with ranks sharing a device: enqueued in lockstep by this thread (group_direct_lockstep)
  const bool lockstep = g->n > 1 && !g->distinct && g->transport == TJ_TRANSPORT_FLAG && g->ctx[0]->d.xch;
  auto run_batch = [&](bool careful, std::vector<long>* extra) {
    if (lockstep && !careful) { if (group_direct_lockstep(g, n_iters, rc)) g->abort_flag.store(1); }
    else if (g->n == 1) rc[0] = group_rank_loop(g, 0, n_iters, careful, extra ? &(*extra)[0] : nullptr);
    else {
      std::vector<std::thread> th;
      for (int r = 0; r < g->n; r++) th.emplace_back([g, r, n_iters, &rc, careful, extra]() { rc[r] = group_rank_loop(g, r, n_iters, careful, extra ? &(*extra)[r] : nullptr); if (rc[r]) g->abort_flag.store(1); });
      for (auto& t : th) t.join();
    }
  };
  run_batch(false, nullptr);
  if (cpl_sharded && std::all_of(rc.begin(), rc.end(), [](int x) { return x == TJ_OK; })) {
    bool range = false;
    for (int r = 0; r < g->n; r++) {
      tj_ctx* c = g->ctx[r];
      int err = 0;
      if (hipSetDevice(g->dev[r]) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(&err, &c->d.ctl->error, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return group_fail(g, TJ_ERR_DEVICE, "tj_group_iterate: reading a rank's error word failed");
      range = range || (err & ERR_LS_RANGE) != 0;
    }
    if (range) {
      // the Armijo search of some iteration needed more candidates than one exchange carries (never met outside constructed states): every rank back to the batch's
      // first state, then the same iterations with the search followed to the reference's own end -- one host look per iteration, slow and exact
      for (int w = 0; w < 5; w++) g->issued[w] += n_iters;   // (the abandoned run's exchanges were issued: the sequence numbers and the buffer parity go on from there)
      for (int r = 0; r < g->n; r++) {
        tj_ctx* c = g->ctx[r];
        (void)hipSetDevice(g->dev[r]);
        if (int e = checkpoint_restore(c)) { g->poisoned = true; return group_fail(g, e, std::string("rank ") + std::to_string(r) + ": " + tj_last_error(c)); }   // (the ranks no longer start from one state)
        tj_set_coupled_follow(c, 1);
      }
      std::vector<long> extra(g->n, 0);
      run_batch(true, &extra);
      for (int r = 0; r < g->n; r++) tj_set_coupled_follow(g->ctx[r], 0);
      g->issued[4] += extra[0];
      g->lsc_followed++;
    }
  }
  for (int r = 0; r < g->n; r++) if (rc[r]) {
    // the ranks have enqueued different numbers of phases and pushes: nothing but tj_group_init_state / destroy may follow
    g->poisoned = true;
    return group_fail(g, rc[r], std::string("rank ") + std::to_string(r) + ": " + tj_last_error(g->ctx[r]));
  }
  {  // what the schedule exchanged, for the parity of the next call
    const bool cpl = g->ctx[0]->d.mode == TJ_MODE_MULTI_COUPLED;
    for (int w = 0; w < (cpl ? 5 : 2); w++) g->issued[w] += n_iters;
  }
  Ctl h0; memset(&h0, 0, sizeof(h0));
  for (int r = 0; r < g->n; r++) {
    tj_ctx* c = g->ctx[r];
    if (hipSetDevice(g->dev[r]) != hipSuccess) return group_fail(g, TJ_ERR_DEVICE, "hipSetDevice failed");
    int e = flush_deferred(c);
    Ctl h;
    if (!e) e = check_device_errors(c, &h);
    if (e) { if (e == TJ_ERR_DEVICE) g->poisoned = true; return group_fail(g, e, std::string("rank ") + std::to_string(r) + ": " + tj_last_error(c)); }
    if (r == 0) h0 = h;   // gnorm, the iteration counter and the stop flag are formed identically on every rank
  }
  const int it = h0.iter + h0.pending;
  if (gnorm) *gnorm = h0.gnorm;
  if (iters_total) *iters_total = it;
  if (converged) *converged = h0.done || (g->ctx[0]->d.stop > 0 && it > 1 && h0.gnorm < g->ctx[0]->d.stop);
  return TJ_OK;
}

// Event-timed cost of ONE exchange of each buffer kind: every rank's host thread issues `reps` exchanges of kind w back to back
// (the slices are what they are: re-sending them changes nothing) between two events on its stream; us[w] = the slowest rank's
// average.  us has 5 entries (kinds 2..4 exist in coupled mode only; 0 otherwise).  One rank: all zeros (nothing is foreign).
int tj_group_profile_exchange(tj_group* g, int reps, double* us) {
  if (!g || !us || reps < 1) return TJ_ERR_INVALID;
  if (g->poisoned) return TJ_ERR_DEVICE;
  for (int w = 0; w < 5; w++) us[w] = 0;
  if (g->n == 1) return TJ_OK;
  const int nwhat = g->ctx[0]->d.mode == TJ_MODE_MULTI_COUPLED ? 5 : 2;
  for (int w = 0; w < nwhat; w++) {
    std::vector<int> rc(g->n, TJ_OK);
    std::vector<float> ms(g->n, 0.f);
    g->abort_flag.store(0);
    std::vector<std::thread> th;
    for (int r = 0; r < g->n; r++) th.emplace_back([g, r, w, reps, &rc, &ms]() {
      tj_ctx* c = g->ctx[r];
      if (hipSetDevice(g->dev[r]) != hipSuccess) { rc[r] = TJ_ERR_DEVICE; g->abort_flag.store(1); return; }
      hipEvent_t e0, e1;
      if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { rc[r] = TJ_ERR_DEVICE; g->abort_flag.store(1); return; }
      long s = g->issued[w];
      int e = group_exchange(g, r, w, s++);   // one untimed exchange first (module load, first-touch of the peer mapping)
      (void)hipEventRecord(e0, c->stream);
      for (int i = 0; i < reps && !e; i++) e = group_exchange(g, r, w, s++);
      (void)hipEventRecord(e1, c->stream);
      if (!e && hipStreamSynchronize(c->stream) != hipSuccess) e = TJ_ERR_DEVICE;
      if (!e) (void)hipEventElapsedTime(&ms[r], e0, e1);
      (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
      rc[r] = e; if (e) g->abort_flag.store(1);
    });
    for (auto& t : th) t.join();
    for (int r = 0; r < g->n; r++) if (rc[r]) { g->poisoned = true; return group_fail(g, rc[r], std::string("rank ") + std::to_string(r) + ": " + tj_last_error(g->ctx[r])); }
    g->issued[w] += reps + 1;
    float worst = 0; for (int r = 0; r < g->n; r++) worst = std::max(worst, ms[r]);
    us[w] = 1e3 * worst / reps;
  }
  return TJ_OK;
}

int tj_group_get_state(tj_group* g, int u, double* spline, double* p_slack, double* p_lambda, double* t_slack, double* t_lambda, double* piece_time) {
  if (!g) return TJ_ERR_INVALID;
  for (int r = 0; r < g->n; r++) {
    tj_ctx* c = g->ctx[r];
    if (u >= c->d.u0 && u < c->d.u1) {
      if (hipSetDevice(g->dev[r]) != hipSuccess) return group_fail(g, TJ_ERR_DEVICE, "hipSetDevice failed");
      const int rc = tj_get_state(c, u, spline, p_slack, p_lambda, t_slack, t_lambda, piece_time);
      if (rc < 0) g->err = tj_last_error(c);
      return rc;
    }
  }
  return group_fail(g, TJ_ERR_INVALID, "tj_group_get_state: no such robot");
}

}  // extern "C" (a template cannot have C linkage)

// A read-only query of every robot by the rank that owns it, the shape of the four tj_group_* queries below: gather, run on every rank, scatter.  A rank holds the OTHER ranks'
// control points as its last exchange left them -- one line search behind the owners after a batch -- and a piece_time for its own robots only, so what the query reads of
// other robots (nets: control points [U][3][T], pts: piece_time [U]) is first read from the owners and handed to every rank: the records are bitwise those of one context.
// run(ctx, net or null, pt or null, part) -> rc; null = the context's own state, which with one rank is current.  rows: per-segment arrays [U][S] as (what run wrote, the
// caller's) to scatter with the owned records, or null pairs.
struct GroupRows { const double* part; double* out; };
// gather and run: each(rank, ctx, net or null, pt or null) -> rc, rank after rank, every rank's device current
template <class Each>
int group_each(tj_group* g, bool nets, bool pts, Each&& each) {
  GROUP_LIVE(g);
  const Dev& d0 = g->ctx[0]->d;
  const int U = d0.U, T = d0.T;
  const bool staged = g->n > 1;
  std::vector<double> net(nets && staged ? (size_t)U * 3 * T : 0), pt(pts && staged ? U : 0);
  for (int u = 0; u < U && (!net.empty() || !pt.empty()); u++) {
    const int rc = tj_group_get_state(g, u, net.empty() ? nullptr : &net[(size_t)u * 3 * T], nullptr, nullptr, nullptr, nullptr, pt.empty() ? nullptr : &pt[u]);
    if (rc < 0) return rc;
  }
  for (int r = 0; r < g->n; r++) {
    tj_ctx* c = g->ctx[r];
    if (hipSetDevice(g->dev[r]) != hipSuccess) return group_fail(g, TJ_ERR_DEVICE, "hipSetDevice failed");
    const int rc = each(r, c, net.empty() ? nullptr : net.data(), pt.empty() ? nullptr : pt.data());
    if (rc < 0) return group_fail(g, rc, std::string("rank ") + std::to_string(r) + ": " + tj_last_error(c));
  }
  return TJ_OK;
}
// scatter: one record per robot (and its rows) from the rank that owns it
template <class Rec, class Run>
int group_query(tj_group* g, bool nets, bool pts, Rec* out, GroupRows rows0, GroupRows rows1, Run&& run) {
  if (!g || !out) return TJ_ERR_INVALID;
  const int U = g->ctx[0]->d.U, S = g->ctx[0]->d.S;
  std::vector<Rec> part(U);
  return group_each(g, nets, pts, [&](int, tj_ctx* c, const double* net, const double* pt) {
    const int rc = run(c, net, pt, part.data());
    if (rc < 0) return rc;
    for (int u = c->d.u0; u < c->d.u1; u++) {
      out[u] = part[u];
      for (const GroupRows& w : {rows0, rows1}) if (w.out) std::copy(w.part + (size_t)u * S, w.part + (size_t)(u + 1) * S, w.out + (size_t)u * S);
    }
    return (int)TJ_OK;
  });
}
// a scratch copy of a per-segment array the caller asked for (null: not asked for, nothing to scatter)
static std::vector<double> group_rows(const tj_group* g, const double* wanted) { return std::vector<double>(g && wanted ? (size_t)g->ctx[0]->d.U * g->ctx[0]->d.S : 0); }

// gather: the rows of a row-listing query, rank after rank.  run(ctx, net, pt, rows or null, room, &count) -> rc is the rank's call with what is left of the caller's rows; it
// leaves in count the rank's rows (negative: not known).  A rank whose rows do not fit writes the first that do and is counted in full; the ranks behind it only count.
// Only THAT capacity error is carried on (the rank set its count above the room it was given, or below zero); any other error ends the group's call with the rank's code.
// state: the ranks read other robots, so the owners' nets and piece times are handed in.  total: the rows of all ranks; unknown: some rank could not count its rows.
template <class Rec, class Run>
int group_gather(tj_group* g, bool state, Rec* rows, int cap, int& total, bool& unknown, Run&& run) {
  if (!g || cap < 0 || (cap > 0 && !rows)) return TJ_ERR_INVALID;
  total = 0; unknown = false;
  return group_each(g, state, state, [&](int, tj_ctx* c, const double* net, const double* pt) {
    const int room = unknown ? 0 : std::max(0, cap - total);
    int nr = 0;
    const int e = run(c, net, pt, room ? rows + total : nullptr, room, &nr);
    if (e < 0 && !(e == TJ_ERR_CAPACITY && (nr > room || nr < 0))) return e;
    if (nr < 0) unknown = true; else total += nr;
    return (int)TJ_OK;
  });
}
// group_gather and its end, for a call whose ranks' rows simply follow one another: *n = the rows of all ranks, and more rows than cap are the group's TJ_ERR_CAPACITY in
// the call's words (what: the window queries' "rows, the caller's hold", or listed_run's) unless the call only counts (no rows)
template <class Rec, class Run>
int group_row_list(tj_group* g, bool state, const char* group_name, Rec* rows, int cap, int* n, Run&& run, const char* what = "rows, the caller's hold") {
  if (!n) return TJ_ERR_INVALID;
  int total; bool unknown;
  const int rc = group_gather(g, state, rows, cap, total, unknown, run);
  if (rc < 0) return rc;
  *n = total;
  if (total > cap && rows) return group_fail(g, TJ_ERR_CAPACITY, std::string(group_name) + ": " + std::to_string(total) + " " + what + " " + std::to_string(cap));
  return TJ_OK;
}
// the rows of a query of listed_run
template <class Q>
int group_listed(tj_group* g, double range, double tol, int max_depth, int max_windows, double extra, typename Q::Rec* rows, int cap, int* n) {
  return group_row_list(g, true, Q::spec.group_name, rows, cap, n, [&](tj_ctx* c, const double* net, const double* pt, typename Q::Rec* out, int room, int* nr) {
    return listed_run<Q>(c, range, tol, max_depth, max_windows, extra, net, pt, out, room, nr); }, "pairs are listed, the caller's rows hold");
}

extern "C" {

int tj_group_audit(tj_group* g, double range, tj_audit_robot* out, double* seg_obs, double* seg_pair) {
  std::vector<double> so = group_rows(g, seg_obs), sp = group_rows(g, seg_pair);
  return group_query(g, true, false, out, {so.data(), seg_obs}, {sp.data(), seg_pair}, [&](tj_ctx* c, const double* net, const double*, tj_audit_robot* part) {
    return audit_run(c, range, net, part, seg_obs ? so.data() : nullptr, seg_pair ? sp.data() : nullptr); });
}

int tj_group_audit_timed(tj_group* g, double range, int levels, tj_audit_timed_robot* out, double* seg_lo, double* seg_hi) {
  std::vector<double> sl = group_rows(g, seg_lo), sh = group_rows(g, seg_hi);
  return group_query(g, true, true, out, {sl.data(), seg_lo}, {sh.data(), seg_hi}, [&](tj_ctx* c, const double* net, const double* pt, tj_audit_timed_robot* part) {
    return audit_timed_run(c, range, levels, net, pt, part, seg_lo ? sl.data() : nullptr, seg_hi ? sh.data() : nullptr); });
}

int tj_group_closest_approach(tj_group* g, double range, double tol, int max_depth, int max_windows, tj_closest_robot* out) {
  return group_query(g, true, true, out, {}, {}, [&](tj_ctx* c, const double* net, const double* pt, tj_closest_robot* part) {
    return closest_run(c, range, tol, max_depth, max_windows, net, pt, part); });
}

// the ranks' lists one after the other: ownership is by contiguous robot blocks in rank order, so that is the (robot, partner) order (tj_path_crossings: the rows
// (u, q > u) by u's owner).  A rank whose rows do not fit writes the first that do and is counted in full; the ranks behind it only count.
int tj_group_pair_approach(tj_group* g, double range, double tol, int max_depth, int max_windows, tj_pair_record* rows, int cap, int* n) { return group_listed<PairQuery>(g, range, tol, max_depth, max_windows, 0.0, rows, cap, n); }
int tj_group_path_crossings(tj_group* g, double range, double tol, int max_depth, int max_windows, tj_crossing_record* rows, int cap, int* n) { return group_listed<CrossQuery>(g, range, tol, max_depth, max_windows, 0.0, rows, cap, n); }
int tj_group_timing_margin(tj_group* g, double dist, double max_slip, double tol, int max_depth, int max_windows, tj_margin_record* rows, int cap, int* n) { return group_listed<MarginQuery>(g, dist, tol, max_depth, max_windows, max_slip, rows, cap, n); }

// tj_proximity_windows, rank after rank: every rank gets the whole `cap` in pair slots and what is left of it in rows.  More pairs than `cap` over the ranks together, as
// one context counts them: *n = -1.  A rank whose rows do not fit writes the first that do and is counted in full; the ranks behind it only count.
int tj_group_proximity_windows(tj_group* g, double dist, double tol, int max_depth, int max_windows, tj_proximity_row* rows, int cap, int* n_pairs, int* n) {
  if (!n || !n_pairs) return TJ_ERR_INVALID;
  int pairs = 0, total; bool unknown;
  const int rc = group_gather(g, true, rows, cap, total, unknown, [&](tj_ctx* c, const double* net, const double* pt, tj_proximity_row* out, int room, int* nr) {
    int np = 0;
    const int e = proximity_run(c, dist, tol, max_depth, max_windows, net, pt, out, cap, room, &np, nr);
    pairs += np;
    return e; });
  if (rc < 0) return rc;
  *n_pairs = pairs;
  *n = unknown || pairs > cap ? -1 : total;
  if (cap == 0 && !rows) return TJ_OK;   // the count-only call
  if (*n < 0) return group_fail(g, TJ_ERR_CAPACITY, "tj_group_proximity_windows: " + std::to_string(pairs) + " pairs are listed, the caller's slots hold " + std::to_string(cap));
  if (total > cap) return group_fail(g, TJ_ERR_CAPACITY, "tj_group_proximity_windows: " + std::to_string(total) + " rows, the caller's hold " + std::to_string(cap));
  return TJ_OK;
}

// from every rank's own state: nothing of another robot is read
int tj_group_obstacle_approach(tj_group* g, double range, double tol, int max_depth, int max_windows, tj_obstacle_robot* out) {
  return group_query(g, false, false, out, {}, {}, [&](tj_ctx* c, const double*, const double*, tj_obstacle_robot* part) {
    return tj_obstacle_approach(c, range, tol, max_depth, max_windows, part); });
}

// tj_obstacle_windows, rank after rank, each from its own state (ownership is by contiguous robot blocks in rank order: that is the (robot, t_first_lo) order).  A rank
// whose rows do not fit writes the first that do and is counted in full; the ranks behind it only count (group_gather).  A walk frontier overflow leaves the rank's
// count untouched and so ends the group's call with the rank's TJ_ERR_CAPACITY, *n untouched.
int tj_group_obstacle_windows(tj_group* g, double dist, double tol, int max_depth, int max_windows, tj_obswin_row* rows, int cap, int* n) {
  return group_row_list(g, false, "tj_group_obstacle_windows", rows, cap, n, [&](tj_ctx* c, const double*, const double*, tj_obswin_row* out, int room, int* nr) {
    return obswin_run(c, dist, tol, max_depth, max_windows, out, room, nr); });
}

// tj_sight_windows, rank after rank with nets and piece_time from the owners: every rank gets the whole link list and answers the links whose robot a it owns, with
// room for the first `cap` of its rows; the host then places the rows link after link -- each link's rows come from one rank, in time order -- which is one
// context's (link, t_first_lo) order.  A rank whose rows exceed `cap` is counted in full.  A walk frontier overflow leaves the rank's count untouched and so ends the
// group's call with the rank's TJ_ERR_CAPACITY, *n untouched.
int tj_group_sight_windows(tj_group* g, const int* links, int n_links, const double* stations, int n_stations, double dist, double tol, int max_depth, int max_windows, tj_sight_row* rows, int cap, int* n) {
  if (!g || !n || cap < 0 || (cap > 0 && !rows)) return TJ_ERR_INVALID;
  std::vector<std::vector<tj_sight_row>> part(g->n);
  std::vector<int> count(g->n, 0);
  const int rc = group_each(g, true, true, [&](int r, tj_ctx* c, const double* net, const double* pt) {
    part[r].resize(cap);
    int nr = -1;
    const int e = sight_run(c, links, n_links, stations, n_stations, dist, tol, max_depth, max_windows, net, pt, cap ? part[r].data() : nullptr, cap, &nr);
    if (e < 0 && !(e == TJ_ERR_CAPACITY && nr > cap)) return e;
    count[r] = nr;
    return (int)TJ_OK;
  });
  if (rc < 0) return rc;
  int total = 0, written = 0;
  for (int r = 0; r < g->n; r++) total += count[r];
  std::vector<int> at(g->n, 0);
  for (int k = 0; k < n_links && written < cap; k++)
    for (int r = 0; r < g->n; r++) {
      if (links[2 * k] < g->ctx[r]->d.u0 || links[2 * k] >= g->ctx[r]->d.u1) continue;
      while (written < cap && at[r] < std::min(count[r], cap) && part[r][at[r]].link == k) rows[written++] = part[r][at[r]++];
    }
  *n = total;
  if (total > cap && !(cap == 0 && !rows)) return group_fail(g, TJ_ERR_CAPACITY, "tj_group_sight_windows: " + std::to_string(total) + " rows, the caller's hold " + std::to_string(cap));
  return TJ_OK;
}

int tj_group_peak_dynamics(tj_group* g, double tol, int max_depth, int max_windows, int length_levels, tj_dynamics_robot* out) {
  return group_query(g, false, false, out, {}, {}, [&](tj_ctx* c, const double*, const double*, tj_dynamics_robot* part) {
    return tj_peak_dynamics(c, tol, max_depth, max_windows, length_levels, part); });
}

// tj_dynamics_windows, rank after rank, each from its own state, without gathered nets (ownership is by contiguous robot blocks in rank order: that is the (robot,
// gate, t_first_lo) order).  A rank whose rows do not fit writes the first that do and is counted in full; the ranks behind it only count (group_gather).
int tj_group_dynamics_windows(tj_group* g, const tj_dyn_gate* gates, int n_gates, double tol, int max_depth, int max_windows, tj_dynwin_row* rows, int cap, int* n) {
  return group_row_list(g, false, "tj_group_dynamics_windows", rows, cap, n, [&](tj_ctx* c, const double*, const double*, tj_dynwin_row* out, int room, int* nr) {
    return dynwin_run(c, gates, n_gates, tol, max_depth, max_windows, out, room, nr); });
}

// tj_zone_windows, rank after rank, each from its own state, without gathered nets: tj_group_dynamics_windows' way, in (robot, zone, t_first_lo) order
int tj_group_zone_windows(tj_group* g, const tj_zone* zones, int n_zones, const double* shapes, int n_shapes, double tol, int max_depth, int max_windows, tj_zonewin_row* rows, int cap, int* n) {
  return group_row_list(g, false, "tj_group_zone_windows", rows, cap, n, [&](tj_ctx* c, const double*, const double*, tj_zonewin_row* out, int room, int* nr) {
    return zonewin_run(c, zones, n_zones, shapes, n_shapes, tol, max_depth, max_windows, out, room, nr); });
}

// the owners' rows [n_times] per robot; control points and piece_time from the owners, so every rank places the whole fleet as one context would
int tj_group_flight_profile(tj_group* g, const double* times, int n_times, tj_profile_sample* out) {
  if (!g || !times || !out || n_times < 1) return TJ_ERR_INVALID;
  const Dev& d0 = g->ctx[0]->d;
  if (n_times > TJ_PROFILE_MAX_SAMPLES || (long long)d0.U * n_times > (long long)TJ_PROFILE_MAX_RECORDS) return TJ_ERR_INVALID;   // (before the scratch copy is sized)
  std::vector<tj_profile_sample> part(g->n > 1 ? (size_t)d0.U * n_times : 0);
  return group_each(g, true, true, [&](int, tj_ctx* c, const double* net, const double* pt) {
    if (part.empty()) return profile_run(c, times, n_times, net, pt, out);
    const int rc = profile_run(c, times, n_times, net, pt, part.data());
    if (rc < 0) return rc;
    std::copy(part.begin() + (size_t)c->d.u0 * n_times, part.begin() + (size_t)c->d.u1 * n_times, out + (size_t)c->d.u0 * n_times);
    return (int)TJ_OK;
  });
}

}  // extern "C"
