// tj_kat.h -- the known-answer hooks of include/trajadmm_kat.h.  TEST BUILD ONLY: tj_api.hip includes this file once, near its end, under TJ_KAT (libtrajadmm_kat.so);
// the product library has none of it.  The hooks run the device primitives of the hot path (kernels_debug.h) on caller-supplied batches, all on one staged path
// (kat_staged), and hand out what the host side knows without a launch: the plan, the launch sequence, the array table, the hull and swept-hull records.
#pragma once

namespace {
constexpr size_t KAT_PT = sizeof(double[3]), KAT_HULL = sizeof(double[6][3]), KAT_TRI = sizeof(double[3][3]);   // a point, a six-vertex hull, a triangle

// one input of a hook: staged where the caller gave it (host != null) or where the kernel wants scratch of that size; else the kernel gets a null pointer
struct KatIn { const void* host; size_t bytes; bool scratch = false; };
struct KatBufs { std::vector<DevBuf> b; const double* operator()(int i) const { return (const double*)b[i].p; } };
// The one path of the batch hooks: stage the inputs, make the output (cleared; preload: then loaded from the caller's, the refine forms' in/out), run
// launch(inputs, output), check the launches, drain the context, copy the output back
template <class Launch>
int kat_staged(tj_ctx* c, std::initializer_list<KatIn> in, void* out, size_t out_bytes, bool preload, Launch&& launch) {
  KatBufs d{std::vector<DevBuf>(in.size())}; DevBuf dout; int r; size_t i = 0;
  for (const KatIn& k : in) { if ((k.host || k.scratch) && (r = to_dev(c, d.b[i], k.host, k.bytes))) return r; i++; }
  if ((r = to_dev(c, dout, nullptr, out_bytes))) return r;
  HIPCHK(c, hipMemsetAsync(dout.p, 0, std::max<size_t>(out_bytes, 8), c->stream));
  if (preload && (r = upload(c, dout.p, out, out_bytes))) return r;
  launch(d, (double*)dout.p);
  HIPCHK(c, hipGetLastError());
  QUIESCE(c);
  HIPCHK(c, hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
  return TJ_OK;
}

// The body sizes the GJK kernels are instantiated for, written once: f(integral_constant n1, integral_constant n2) for the pair (n1, n2) if it is one of MASK's
// (bit i = kBodies[i]); false: it is not.  A hook names its subset, and its error text is built from that subset (bodies_error)
struct Bodies { int n1, n2; };
constexpr Bodies kBodies[6] = {{6, 1}, {6, 3}, {6, 6}, {12, 1}, {12, 3}, {12, 12}};
constexpr unsigned BODIES_ALL = 63, BODIES_SQUARE = 1u << 2 | 1u << 5;
template <unsigned MASK, int I = 0, class F>
bool with_bodies(int n1, int n2, F&& f) {
  if constexpr (I < 6) {
    if constexpr ((MASK >> I) & 1)
      if (n1 == kBodies[I].n1 && n2 == kBodies[I].n2) { f(std::integral_constant<int, kBodies[I].n1>{}, std::integral_constant<int, kBodies[I].n2>{}); return true; }
    return with_bodies<MASK, I + 1>(n1, n2, f);
  }
  return false;
}
int bodies_error(tj_ctx* c, const char* who, unsigned mask) {
  c->err = std::string(who) + ": body sizes must be ";
  for (int i = 0, left = __builtin_popcount(mask); i < 6; i++)
    if ((mask >> i) & 1) { left--; c->err += std::to_string(kBodies[i].n1) + "v" + std::to_string(kBodies[i].n2) + (left > 1 ? ", " : (left == 1 ? " or " : "")); }
  return TJ_ERR_INVALID;
}

// the three GJK hooks: a[n][n1][3] and b[n][n2][3] in, `scratch` doubles per case next to them, `per` doubles per case out; launch(N1, N2, inputs, out) for a pair of MASK's
template <unsigned MASK, class Launch>
int kat_gjk_run(tj_ctx* c, const char* who, int n, int n1, const double* a, int n2, const double* b, size_t scratch, double* out, size_t per, Launch&& launch) {
  if (!c || n < 0 || !a || !b || !out) return TJ_ERR_INVALID;
  if (!with_bodies<MASK>(n1, n2, [](auto, auto) {})) return bodies_error(c, who, MASK);
  return kat_staged(c, {{a, (size_t)n * n1 * KAT_PT}, {b, (size_t)n * n2 * KAT_PT}, {nullptr, n * scratch * sizeof(double), scratch > 0}}, out, n * per * sizeof(double), false,
                    [&](const KatBufs& d, double* o) { with_bodies<MASK>(n1, n2, [&](auto N1, auto N2) { launch(N1, N2, d, o); }); });
}

// The walk reports a frontier overflow to the queries' control block (walk_dev), as every read-only query does: a deliberate overflow here is this call's error
// and leaves the solver's error word, and with it the context, as it was.  `who`: the entry point the call came in through (the error texts name it).
// (Not on the staged path: the context is drained BEFORE the walk, and the walk's end is the queries'.)
int kat_query_run(tj_ctx* c, const char* who, int nq, const double* boxes, double margin, int cap, int unroll, int pre, int* counts, int* ids) {
  if (!c || nq < 0 || cap < 1 || !boxes || !counts || !ids || (unroll != 1 && unroll != 4)) return TJ_ERR_INVALID;
  if (!c->have_cloud) { c->err = std::string(who) + ": set the obstacles first"; return TJ_ERR_INVALID; }
  DevBuf db, di, dn; int r;
  if ((r = to_dev(c, db, boxes, (size_t)nq * sizeof(double[6]))) || (r = to_dev(c, di, nullptr, (size_t)nq * cap * sizeof(int))) || (r = to_dev(c, dn, nullptr, (size_t)nq * sizeof(int)))) return r;
  QUIESCE(c);
  Dev da;
  if ((r = walk_dev(c, da))) return r;
  with_prim(c->d, [&](auto prim) {
    constexpr int PR = decltype(prim)::value;
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(std::max(nq, 1)), dim3(64), 0, c->stream, da, nq, (const double*)db.p, margin, cap, (int*)di.p, (int*)dn.p); };
    if (unroll == 4) { if (pre) go(k_dbg_query<PR, 4, true>); else go(k_dbg_query<PR, 4, false>); }
    else { if (pre) go(k_dbg_query<PR, 1, true>); else go(k_dbg_query<PR, 1, false>); }
  });
  if ((r = query_finish(c, who))) {
    if (r == TJ_ERR_CAPACITY)   // (query_finish words it for a trajectory query: a segment and a `range`; here the caller gave boxes and a margin)
      c->err = std::string(who) + ": the BVH frontier of one of the " + std::to_string(nq) + " query boxes overflowed at margin " + std::to_string(margin) + " (more than " + std::to_string(FRONT_CAP) +
               " boxes of one level within the margin of the query box): ask with smaller boxes or a smaller margin";
    return r;
  }
  if (nq == 0) return TJ_OK;
  HIPCHK(c, hipMemcpy(counts, dn.p, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(ids, di.p, (size_t)nq * cap * sizeof(int), hipMemcpyDeviceToHost));
  for (int q = 0; q < nq; q++) {
    if (counts[q] > cap) { c->err = std::string(who) + ": query box " + std::to_string(q) + " returned " + std::to_string(counts[q]) + " candidates, more than cap = " + std::to_string(cap); return TJ_ERR_CAPACITY; }
    ids_to_caller(c, ids + (size_t)q * cap, std::max(counts[q], 0));
  }
  return check_device_errors(c);
}

// a cache of padded records as its last writer left it: fetched whole, the first `rec` doubles of every `stride` handed out; then its box table.  No kernel runs
int kat_records(tj_ctx* c, double* Dev::*info, size_t stride, size_t rec, double* out, double* Dev::*boxes, double* box) {
  if (!c || !out || !box || !ready(c)) return TJ_ERR_INVALID;
  QUIESCE(c);
  std::vector<double> h(array_count(c, c->d.*info)); int r;
  if ((r = fetch(c, h.data(), c->d.*info, 0, h.size()))) return r;
  for (size_t i = 0; i < h.size() / stride; i++) memcpy(out + i * rec, h.data() + i * stride, rec * sizeof(double));
  return fetch(c, box, c->d.*boxes, 0, array_count(c, c->d.*boxes));
}

// what a hook without a launch looks at (tj_kat_plan, tj_kat_launches, tj_kat_arrays): a context's own Dev, plan and facts, or -- c == nullptr, no device needed -- the
// pure planner's on the caller's parameters and PLAN_FACT_INTS device facts.  false: a shape the planner refuses (pl.err, pl.msg say why)
bool kat_source(const tj_ctx* c, const tj_params* p, const int* facts, Plan& pl, PlanFacts& f) {
  if (c) { pl.d = c->d; pl.h = c->hp; f = c->facts; f.prim = c->d.prim; f.n_obs = c->d.N; return true; }
  memcpy(&f, facts, sizeof(f));
  if (const char* bad = plan_check_params(p)) { pl.err = TJ_ERR_INVALID; pl.msg = bad; memset(&pl.d, 0, sizeof(pl.d)); pl.h.lsl = LsLayout{}; return false; }
  pl = plan_context(p, f, tune); pl.d.prim = f.prim; pl.d.N = f.n_obs;
  return !pl.err;
}

}  // namespace

extern "C" {
int tj_kat_gjk(tj_ctx* c, int n, int n1, const double* a, int n2, const double* b, double* v) {
  return kat_gjk_run<BODIES_ALL>(c, "tj_kat_gjk", n, n1, a, n2, b, 0, v, 3, [&](auto N1, auto N2, const KatBufs& d, double* o) {
    hipLaunchKernelGGL((k_dbg_gjk<decltype(N1)::value, decltype(N2)::value>), dim3((n + 63) / 64), dim3(64), 0, c->stream, n, d(0), d(1), o);
  });
}
int tj_kat_gjk_wave(tj_ctx* c, int n, int n1, const double* a, int n2, const double* b, double* v) {
  return kat_gjk_run<BODIES_ALL>(c, "tj_kat_gjk_wave", n, n1, a, n2, b, 0, v, 3, [&](auto N1, auto N2, const KatBufs& d, double* o) {
    hipLaunchKernelGGL((k_dbg_gjk_wave<decltype(N1)::value, decltype(N2)::value>), dim3(std::max(n, 1)), dim3(64), 0, c->stream, n, d(0), d(1), o);
  });
}
int tj_kat_gjk_wave_split(tj_ctx* c, int n, int n1, const double* a, int n2, const double* b, int k_stop, double* v_iters) {
  if (k_stop < 1) return TJ_ERR_INVALID;   // (scratch: a case's loop state between the two halves, 32 doubles)
  return kat_gjk_run<BODIES_SQUARE>(c, "tj_kat_gjk_wave_split", n, n1, a, n2, b, 32, v_iters, 4, [&](auto N1, auto N2, const KatBufs& d, double* o) {
    hipLaunchKernelGGL((k_dbg_gjk_wave_split<decltype(N1)::value, decltype(N2)::value>), dim3(std::max(n, 1)), dim3(64), 0, c->stream, n, d(0), d(1), k_stop, (double*)d(2), o);
  });
}

int tj_kat_planes(tj_ctx* c, int what, int n, const double* P, const double* Q, double dist, double* out) {
  if (!c || n < 0 || what < 0 || what > 7 || !P || !Q || !out) return TJ_ERR_INVALID;
  const size_t qbytes = (size_t)n * ((what == 0 || what == 2 || what == 5) ? KAT_PT : KAT_HULL);  // what 1, 3, 4, 6: hull vs hull
  // (what >= 5: in/out, the plane to refine)
  return kat_staged(c, {{P, (size_t)n * KAT_HULL}, {Q, qbytes}}, out, (size_t)n * sizeof(double[5]), what >= 5, [&](const KatBufs& d, double* o) {
    const dim3 waves(std::max(n, 1)), lanes((n + 63) / 64), t(64);
    if (what == 7) hipLaunchKernelGGL(k_dbg_optpair_wave, waves, t, 0, c->stream, c->d, n, d(0), d(1), o);
    else if (what == 2) hipLaunchKernelGGL((k_dbg_kdop_wave<1, false>), waves, t, 0, c->stream, c->d, n, d(0), nullptr, nullptr, d(1), 1, nullptr, dist, o, 5);
    else if (what == 4) hipLaunchKernelGGL(k_dbg_pair_wave, waves, t, 0, c->stream, c->d, n, d(0), d(1), dist, o);
    else hipLaunchKernelGGL(k_dbg_planes, lanes, t, 0, c->stream, c->d, what, n, d(0), d(1), dist, o);
  });
}

int tj_kat_ccd(tj_ctx* c, int n, const double* P, const double* D, const double* Q, const double* E, const double* q, const double* tu, double d, double* out) {
  if (!c || n < 0 || !P || !D || !Q || !E || !q || !tu || !out) return TJ_ERR_INVALID;
  const size_t hulls = (size_t)n * KAT_HULL;
  return kat_staged(c, {{P, hulls}, {D, hulls}, {Q, hulls}, {E, hulls}, {q, (size_t)n * KAT_PT}, {tu, (size_t)n * sizeof(double[2])}}, out, (size_t)n * sizeof(double[2]), false,
                    [&](const KatBufs& b, double* o) {
    hipLaunchKernelGGL(k_dbg_ccd, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, b(0), b(1), b(2), b(3), b(4), b(5), d, o);
  });
}

int tj_kat_query_form(tj_ctx* c, int nq, const double* boxes, double margin, int cap, int unroll, int pre, int* counts, int* ids) {
  return kat_query_run(c, "tj_kat_query_form", nq, boxes, margin, cap, unroll, pre, counts, ids);
}
int tj_kat_query(tj_ctx* c, int nq, const double* boxes, double margin, int cap, int* counts, int* ids) {   // the plane query's form, no prefetched top box
  return kat_query_run(c, "tj_kat_query", nq, boxes, margin, cap, 4, 0, counts, ids);
}

int tj_kat_tri(tj_ctx* c, int n, const double* P, const double* D, const double* tri, const double* t, double dist, double off, double* out) {
  if (!c || n < 0 || !P || !D || !tri || !t || !out) return TJ_ERR_INVALID;
  return kat_staged(c, {{P, (size_t)n * KAT_HULL}, {D, (size_t)n * KAT_HULL}, {tri, (size_t)n * KAT_TRI}, {t, (size_t)n * sizeof(double)}}, out, (size_t)n * sizeof(double[8]), false,
                    [&](const KatBufs& b, double* o) {
    hipLaunchKernelGGL(k_dbg_tri, dim3((n + 63) / 64), dim3(64), 0, c->stream, c->d, n, b(0), b(1), b(2), b(3), dist, off, o);
    // the two k-DOP verdicts, out[.][5] and out[.][6]: one wave per case, the triangle on lane 0
    hipLaunchKernelGGL((k_dbg_kdop_wave<3, false>), dim3(std::max(n, 1)), dim3(64), 0, c->stream, c->d, n, b(0), nullptr, nullptr, b(2), 1, nullptr, dist, o + 5, 8);
    hipLaunchKernelGGL((k_dbg_kdop_wave<3, true>), dim3(std::max(n, 1)), dim3(64), 0, c->stream, c->d, n, b(0), b(1), b(3), b(2), 1, nullptr, off, o + 6, 8);
  });
}

int tj_kat_kdop_wave(tj_ctx* c, int prim, int swept, int n, int per, const double* P, const double* D, const double* t, const double* bodies, const int* nc, double d, double* out) {
  if (!c || n < 0 || per < 1 || per > 64 || (prim != 1 && prim != 3) || !P || !bodies || !out || (swept && (!D || !t))) return TJ_ERR_INVALID;
  return kat_staged(c, {{P, (size_t)n * KAT_HULL}, {swept ? D : nullptr, (size_t)n * KAT_HULL}, {swept ? t : nullptr, (size_t)n * sizeof(double)}, {bodies, (size_t)n * per * prim * KAT_PT},
                        {nc, (size_t)n * sizeof(int)}}, out, (size_t)n * per * sizeof(double), false, [&](const KatBufs& b, double* o) {
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(std::max(n, 1)), dim3(64), 0, c->stream, c->d, n, b(0), b(1), b(2), b(3), per, (const int*)b.b[4].p, d, o, 1); };
    if (prim == 1) { if (swept) go(k_dbg_kdop_wave<1, true>); else go(k_dbg_kdop_wave<1, false>); }
    else { if (swept) go(k_dbg_kdop_wave<3, true>); else go(k_dbg_kdop_wave<3, false>); }
  });
}

// the launch plan as a flat record of ints (host_plan.h: plan_record).  Returns the number of ints (negated: `cap` is too small), msg: the planner's error text
int tj_kat_plan(const tj_ctx* c, const tj_params* p, const int* facts, int* out, int cap, char* msg, int msg_cap) {
  if (!out || (!c && (!p || !facts))) return 0;
  Plan pl; PlanFacts f;
  kat_source(c, p, facts, pl, f);   // (a refused shape is a record too: its `err` entry and msg)
  if (msg && msg_cap > 0) { strncpy(msg, pl.msg, (size_t)msg_cap - 1); msg[msg_cap - 1] = 0; }
  return plan_record(pl, f, out, cap);
}

// the launch sequence as flat records of ints (host_launch.h: sequence_kernel), call by call, from a context's state (copied to `state` first, but for xs_same_queue_now,
// and not advanced) or the start state in `state`.  calls: n_calls x (kid, sched, chain_pos).  out, per call: exists, number of records, the SchedState after it, the
// Launch records.  Returns the ints written (negated: `cap` is too small; 0: bad arguments or a shape the planner refuses)
int tj_kat_launches(const tj_ctx* c, const tj_params* p, const int* facts, int lsc_follow, int* state, const int* calls, int n_calls, int* out, int cap) {
  if (!out || !state || n_calls < 0 || (n_calls > 0 && !calls) || (!c && (!p || !facts))) return 0;
  Plan pl; PlanFacts f; SchedState st;
  if (!kat_source(c, p, facts, pl, f)) return 0;
  memcpy(&st, state, sizeof(st));
  if (c) { const int same = st.xs_same_queue_now ? 1 : 0; st = c->ss; st.xs_same_queue_now = same; memcpy(state, &st, sizeof(st)); }   // (xs_same_queue_now comes FROM state[]: tj_profile_kernels sets it around its run only, so the caller says which run it asks about)
  else pl.d.lsc_follow = lsc_follow ? 1 : 0;
  int n = 0;
  for (int i = 0; i < n_calls; i++) {
    const int kid = calls[3 * i], sched = calls[3 * i + 1];
    if (kid < 0 || kid >= K_COUNT || sched < 0 || sched > 2) return 0;
    LaunchList l;
    const bool exists = sequence_kernel(pl.d, pl.h, st, (Sched)sched, calls[3 * i + 2], kid, l);
    const int need = 2 + SCHED_STATE_INTS + l.n * LAUNCH_INTS;
    if (n + need > cap) return -(n + need);
    out[n] = exists ? 1 : 0; out[n + 1] = l.n;
    memcpy(out + n + 2, &st, sizeof(st)); memcpy(out + n + 2 + SCHED_STATE_INTS, l.v, (size_t)l.n * sizeof(Launch));
    n += need;
  }
  return n;
}

// the declaration table of the device arrays (tj_api.hip: device_arrays), four ints per array -- element count, element size, checkpoint flag, reset kind (0 none,
// 1 zero bytes, 2 one bytes) -- and the names, comma-joined.  Returns the number of arrays (negated: cap ints or names_cap chars are too few; 0: bad arguments or a refused shape)
int tj_kat_arrays(const tj_ctx* c, const tj_params* p, const int* facts, int* out, int cap, char* names, int names_cap) {
  if (!out || !names || (!c && (!p || !facts))) return 0;
  Plan pl; PlanFacts f;
  if (!kat_source(c, p, facts, pl, f)) return 0;
  const std::vector<ArrayDecl> a = c ? c->arrays : device_arrays(pl.d);
  std::string all;
  for (const ArrayDecl& e : a) all += (all.empty() ? "" : ",") + std::string(e.name);
  const int n = (int)a.size();
  if (4 * n > cap || (int)all.size() + 1 > names_cap) return -n;
  for (int i = 0; i < n; i++) { out[4 * i] = (int)a[i].n; out[4 * i + 1] = (int)a[i].elem; out[4 * i + 2] = a[i].snap; out[4 * i + 3] = a[i].reset == ONES ? 2 : (a[i].reset == ZERO ? 1 : 0); }
  memcpy(names, all.c_str(), all.size() + 1);
  return n;
}

int tj_kat_linalg(tj_ctx* c, int nmat, int n, const double* mats, double* out) {
  if (!c || nmat < 0 || n < 1 || n > 64 || !mats || !out) return TJ_ERR_INVALID;
  return kat_staged(c, {{mats, (size_t)nmat * n * n * sizeof(double)}}, out, (size_t)nmat * sizeof(double[2]), false, [&](const KatBufs& d, double* o) {
    hipLaunchKernelGGL(k_dbg_linalg, dim3(nmat), dim3(64), (2 * (size_t)n * n + 4 * n) * sizeof(double), c->stream, nmat, n, d(0), o);
  });
}

// the counterpart of tj_get_local_grad for the whole fleet: the per-piece blocks k_xsolve / k_xsolve_band read, from the host.  No kernel runs
int tj_kat_set_local_grad(tj_ctx* c, const double* lg, const double* lh) {
  if (!c || !lg || !lh || !ready(c)) return TJ_ERR_INVALID;
  QUIESCE(c);
  const int r = store(c, c->d.lg, 0, lg, array_count(c, c->d.lg));
  return r ? r : store(c, c->d.lh, 0, lh, array_count(c, c->d.lh));
}

// the hull cache as the last launch that wrote it left it: the 122 values of every (robot, segment) record and the box table
int tj_kat_get_hull_record(tj_ctx* c, double* hullinfo, double* hbox) { return kat_records(c, &Dev::hullinfo, HULL_INFO_STRIDE, 122, hullinfo, &Dev::hbox, hbox); }
// the swept-hull cache likewise: the CCD_REC values of every (robot, segment) record and the pair-box table
int tj_kat_get_swept_record(tj_ctx* c, double* ccdinfo, double* cbox) { return kat_records(c, &Dev::ccdinfo, CCD_STRIDE, CCD_REC, ccdinfo, &Dev::cbox, cbox); }

}  // extern "C"
