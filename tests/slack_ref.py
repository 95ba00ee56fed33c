"""One piece's slack (z) and dual update, twice over -- TEST INFRASTRUCTURE ONLY.

  truth      mpmath at DPS = 60 digits, every constant an exact rational (1.1 = 11/10, 0.95 = 19/20, 0.8 = 4/5, 1e-4 = 1/10000), mpmath.eigsy for the eigenvalue.
  yardstick  the same formulas in plain fp64 in the natural loop order, with the fp64 constants: the answer of someone who did not try to be clever.  Its distance from
             the truth says what fp64 costs on these inputs; the device is held to a multiple of it (tests/test_gpu_slack.py).
  faults     eight one-line faults that can be planted in the yardstick (FAULTS); tests/test_slack_ref.py shows that each misses the bars.

The update is restated from the formulas the kernel cites (slack_body in csrc/kernels_step.h; Energy_admm.h:172-215, Gradient_admm.h:574-671, update_slack_lambda), not from the
device's order of operations.  Piece sp of a robot has the slack block z[j + 6 a] (control point j < 6, axis a < 3), the time slack t, their duals Lambda, lambda_t, and sees the
spline through cx = C x (C = convert[sp], x[k][a] = net[3 sp + k][a]) and the flight time pt = piece_time:

  E(z, t) = ks / (2 t^5) sum_a z_a^T M z_a + kt t^1.1 + mu/2 |cx - z|^2 + mu/2 (pt - t)^2 + Lambda . (cx - z) + lambda_t (pt - t)            (M = mdyn, symmetric)

With g1 = ks/t^5 M z_a, dyn = the first term: dE/dz = g1 + mu (z - cx) - Lambda, dE/dt = -5 dyn/t + 1.1 kt t^0.1 + mu (t - pt) - lambda_t, d2E/dz2 = ks/t^5 M + mu I per axis,
d2E/dzdt = -5 g1/t, d2E/dt2 = 30 dyn/t^2 + 0.11 kt t^-0.9 + mu (unknown 3 k + a for z[k + 6 a], 18 for t).  The first piece keeps its control points 0, 1 fixed (lo = 2), the
last one 4, 5 (lo = 0): n = 13 unknowns, else n = 19.  If the reduced Hessian is not positive definite and its smallest eigenvalue ev < 0, sigma = -ev + 0.01 is added to its
diagonal.  x = -(H + sigma I)^-1 g, wolfe = -x . g, step0 = 1 -- or -0.95 t / x_t if t + x_t <= 0 (the guard) --, step = step0 0.8^k for the first k with
NOT e - 1e-4 wolfe step < E(z + step x_z, t + step x_t); then z' = z + step x_z, t' = t + step x_t, Lambda' = Lambda + mu (cx - z'), lambda_t' = lambda_t + mu (pt - t').

Undecidable pieces (left out of the outcome assertions): (i) the truth's smallest eigenvalue within the project's eigenvalue bar EIG_BAR max(1, |H|_max) of 0; (ii) an Armijo
comparison up to the accepted one whose margin is below K times what fp64 costs on the two energies: |yardstick - truth| of each, floored at u times the energy's magnitude sum
(the yardstick's candidate energy is taken at ITS direction, so this holds the direction's error as well).

The repair.  A repaired piece's shift is the eigenvalue of the program's OWN matrix, held by the project to the eigenvalue bar only, and the shifted matrix's smallest eigenvalue is
0.01: x moves by dsigma dx/dsigma, dx/dsigma = -(H + sigma I)^-1 x as large as 100 |x|.  A flat allowance of bar |dx/dsigma| would swallow the update wherever |H|_max reaches 1e10
(t_slack scaled by 0.01: the bar exceeds 0.01 itself).  So the allowance is taken in its sharpest form: fit_shift() finds the ONE dsigma, at most the eigenvalue bar in size, at
which the truth's shifted solve comes closest to the outputs measured, and the outputs are measured against the truth at sigma + dsigma: 13 or 19 numbers against one free
parameter.  The fitted dsigma over the bar is returned next to the error.

Error measure (measure()): per piece ||delta - delta_truth||_2 / ||delta_truth||_2 for delta = (z' - z, t' - t), the denominator floored at u ||(z, t)||; the dual blocks the same
with delta = (Lambda' - Lambda, lambda_t' - lambda_t), the numerator less the one rounding of Lambda + mu (C x - z') (u ||(Lambda', lambda_t')||) when a value is held to the bar.
r_class = the yardstick's worst over a class at a shape -- its dual with that rounding left in --, floored at u; a value is accepted within K r_class, K = 8 (bars(), inside()).
"""
import math

import numpy as np
from mpmath import mp, mpf, eigsy, matrix

DPS = 60
U64 = 2.0 ** -53
EIG_BAR = 1e-12      # the project's eigenvalue bar: 1e-12 max(1, |H|_max)
K = 8.0
LOOP_CAP = 400
FAULTS = ("cross4", "corner20", "kt010", "lo_swap", "shift001", "guard1", "dual_prez", "backoff05")


class _F:      # the yardstick's arithmetic
    num = float
    pow = staticmethod(math.pow)

    @staticmethod
    def q(a, b):
        return a / b


class _M:      # the truth's
    num = staticmethod(mpf)
    pow = staticmethod(mp.power)

    @staticmethod
    def q(a, b):
        return mpf(a) / b


_TABLES = {}


def problem(pkg, params, ks, P, st, u, sp):
    """one piece's inputs: the robot's control net, convert[sp], mdyn, ks, kt, mu, piece_time, the piece's z, Lambda, t_z, lambda_t"""
    if P not in _TABLES:
        _TABLES[P] = pkg.host_tables(P, params["res"])[:2]
    conv, M = _TABLES[P]
    return dict(sp=sp, P=P, ks=float(ks), kt=float(params["kt"]), mu=float(params["mu"]), pt=float(st["piece_time"][u]), C=conv[sp], M=M,
                x=[[float(st["spline"][u][a][3 * sp + k]) for a in range(3)] for k in range(6)],
                z=[float(st["p_slack"][u][a][6 * sp + j]) for a in range(3) for j in range(6)],
                lam=[float(st["p_lambda"][u][a][6 * sp + j]) for a in range(3) for j in range(6)],
                tz=float(st["t_slack"][u][sp]), lt=float(st["t_lambda"][u][sp]))


def problems(pkg, params, ks, P, st):
    return [[problem(pkg, params, ks, P, st, u, sp) for sp in range(P)] for u in range(st["t_slack"].shape[0])]


def unknowns(sp, P, fault=None):
    """(lo, tn, the reduced system's unknowns among the 19): boundary pieces keep two control points fixed"""
    lo, tn = 0, 6
    first, last = (sp == P - 1, sp == 0) if fault == "lo_swap" else (sp == 0, sp == P - 1)
    if first:
        lo, tn = 2, 4
    elif last:
        lo, tn = 0, 4
    return lo, tn, [3 * lo + i for i in range(3 * tn)] + [18]


# ---- the formulas, once, over an arithmetic ---------------------------------------------------------------------------------------------
def _inputs(ar, pr):
    c = {k: ar.num(pr[k]) for k in ("ks", "kt", "mu", "pt", "tz", "lt")}
    c["M"] = [[ar.num(v) for v in row] for row in pr["M"]]
    c["z"] = [ar.num(v) for v in pr["z"]]
    c["lam"] = [ar.num(v) for v in pr["lam"]]
    C = [[ar.num(v) for v in row] for row in pr["C"]]
    cx = []
    for a in range(3):
        for j in range(6):
            acc = ar.num(0)
            for k in range(6):
                acc += C[j][k] * ar.num(pr["x"][k][a])
            cx.append(acc)
    c["cx"] = cx
    return c


def _dyn(ar, c, z, t):
    """(ks / (2 t^5) sum_a z_a^T M z_a, its magnitude sum)"""
    s = c["ks"] / t ** 5 / 2
    M = c["M"]
    q, A = ar.num(0), 0.0
    for a in range(3):
        for j in range(6):
            y = ar.num(0)
            for k in range(6):
                y += z[k + 6 * a] * M[k][j]
            q += y * z[j + 6 * a]
    if "Mabs" not in c:
        c["Mabs"] = [[abs(float(v)) for v in row] for row in M]
    zf, Mf = [abs(float(v)) for v in z], c["Mabs"]
    for a in range(3):
        for j in range(6):
            for k in range(6):
                A += zf[k + 6 * a] * Mf[k][j] * zf[j + 6 * a]
    return s * q, abs(float(s)) * A


def _energy(ar, c, z, t):
    """(E(z, t), its magnitude sum)"""
    e, A = _dyn(ar, c, z, t)
    term = c["kt"] * ar.pow(t, ar.q(11, 10))
    e += term; A += abs(float(term))
    mu, cx, lam, pt = c["mu"], c["cx"], c["lam"], c["pt"]
    sq, Asq = ar.num(0), 0.0
    for i in range(18):
        d = cx[i] - z[i]
        sq += d * d
        Asq += abs(float(d)) * (abs(float(cx[i])) + abs(float(z[i])))
    e += mu / 2 * sq; A += float(mu) / 2 * Asq
    dt = pt - t
    e += mu / 2 * (dt * dt); A += float(mu) / 2 * abs(float(dt)) * (abs(float(pt)) + abs(float(t)))
    for i in range(18):
        e += lam[i] * (cx[i] - z[i]); A += abs(float(lam[i])) * (abs(float(cx[i])) + abs(float(z[i])))
    e += c["lt"] * dt; A += abs(float(c["lt"])) * (abs(float(pt)) + abs(float(t)))
    return e, A


def _grad_hess(ar, c, z, t, fault=None):
    """(g[19], H[19][19]) of E at (z, t)"""
    z0 = ar.num(0)
    M, mu, cx, lam = c["M"], c["mu"], c["cx"], c["lam"]
    sc = c["ks"] / t ** 5
    dyn, _ = _dyn(ar, c, z, t)
    g, H = [z0] * 19, [[z0] * 19 for _ in range(19)]
    for k in range(6):
        for a in range(3):
            mz = ar.num(0)
            for j in range(6):
                mz += M[k][j] * z[j + 6 * a]
            g1 = sc * mz
            i = 3 * k + a
            g[i] = g1 + (mu * (z[k + 6 * a] - cx[k + 6 * a]) - lam[k + 6 * a])
            H[i][18] = H[18][i] = -(4 if fault == "cross4" else 5) * g1 / t
            for b in range(6):
                H[i][3 * b + a] = sc * M[k][b] + (mu if k == b else z0)
    g[18] = -5 * dyn / t + c["kt"] * ar.q(11, 10) * ar.pow(t, ar.q(1, 10)) + mu * (t - c["pt"]) - c["lt"]
    H[18][18] = (20 if fault == "corner20" else 30) * dyn / (t * t) + c["kt"] * (ar.q(1, 10) if fault == "kt010" else ar.q(11, 100)) * ar.pow(t, ar.q(-9, 10)) + mu
    return g, H


def _search(ar, c, pr, x, idx, lo, tn, g, fault=None, kmin=0, force_k=None):
    """the step from the direction x (reduced unknowns): guard, Armijo back-offs, the four outputs.  kmin: evaluate the candidates up to 0.8^kmin even beyond the accepted one"""
    z, t = c["z"], c["tz"]
    n = len(idx)
    wolfe = ar.num(0)
    for i in range(n):
        wolfe += x[i] * g[i]
    wolfe = -wolfe
    dirz = [ar.num(0)] * 18
    for i in range(tn):
        for a in range(3):
            dirz[(lo + i) + 6 * a] = x[3 * i + a]
    t_dir = x[n - 1]
    step = ar.num(1)
    guard = bool(t + step * t_dir <= 0)
    if guard:
        step = -(ar.num(1) if fault == "guard1" else ar.q(19, 20)) * t / t_dir
    step0 = step
    if force_k is not None:      # the outputs at 0.8^force_k, no energies
        for _ in range(force_k):
            step = step * ar.q(4, 5)
        trials, acc, e0, A0 = {force_k: dict(step=step, z=[z[i] + step * dirz[i] for i in range(18)], t=t + step * t_dir)}, force_k, None, None
    else:
        e0, A0 = _energy(ar, c, z, t)
        trials, k, acc = [], 0, None
        while True:
            zt = [z[i] + step * dirz[i] for i in range(18)]
            tt = t + step * t_dir
            en, An = _energy(ar, c, zt, tt)
            lhs = e0 - ar.q(1, 10000) * wolfe * step
            trials.append(dict(step=step, en=en, A=An, margin=en - lhs, z=zt, t=tt))
            if acc is None and (not lhs < en or k >= LOOP_CAP):
                acc = k
            if acc is not None and k >= kmin:
                break
            step = step * (ar.q(1, 2) if fault == "backoff05" else ar.q(4, 5)); k += 1
    zt, tt = trials[acc]["z"], trials[acc]["t"]
    mu, cx = c["mu"], c["cx"]
    zd = z if fault == "dual_prez" else zt
    lam1 = [c["lam"][i] + mu * (cx[i] - zd[i]) for i in range(18)]
    lt1 = c["lt"] + mu * (c["pt"] - tt)
    return dict(wolfe=wolfe, t_dir=t_dir, dirz=dirz, guard=guard, step0=step0, k=acc, step=trials[acc]["step"], e0=e0, A0=A0, trials=trials, z1=zt, t1=tt, lam1=lam1, lt1=lt1)


# ---- public: truth ------------------------------------------------------------------------------------------------------------------------
def energy(pr, z=None, t=None, dps=DPS):
    """the truth's E (mpf) at the piece's (z, t) or at the ones given"""
    with mp.workdps(dps):
        c = _inputs(_M, pr)
        return _energy(_M, c, c["z"] if z is None else z, c["tz"] if t is None else t)[0]


def grad_hess(pr, dps=DPS):
    """the truth's full gradient (19) and Hessian (19 x 19)"""
    with mp.workdps(dps):
        c = _inputs(_M, pr)
        return _grad_hess(_M, c, c["z"], c["tz"])


def fd_grad_hess(pr, h=mpf("1e-25"), dps=80):
    """central differences of the truth's energy over all 19 unknowns"""
    with mp.workdps(dps):
        c = _inputs(_M, pr)

        def E(moves):
            z = c["z"][:]; t = c["tz"]
            for i, s in moves:
                if i == 18:
                    t = t + s * h
                else:
                    z[i // 3 + 6 * (i % 3)] = z[i // 3 + 6 * (i % 3)] + s * h
            return _energy(_M, c, z, t)[0]
        e0 = E(())
        g, H = [None] * 19, [[None] * 19 for _ in range(19)]
        ep = [E(((i, 1),)) for i in range(19)]; em = [E(((i, -1),)) for i in range(19)]
        for i in range(19):
            g[i] = (ep[i] - em[i]) / (2 * h)
            H[i][i] = (ep[i] - 2 * e0 + em[i]) / (h * h)
            for k in range(i):
                H[i][k] = H[k][i] = (E(((i, 1), (k, 1))) - E(((i, 1), (k, -1))) - E(((i, -1), (k, 1))) + E(((i, -1), (k, -1)))) / (4 * h * h)
        return g, H


def min_eig(pr, dps=DPS):
    """the truth's smallest eigenvalue of the reduced Hessian (mpf) and its eigenvalue bar"""
    with mp.workdps(dps):
        c = _inputs(_M, pr)
        _, H = _grad_hess(_M, c, c["z"], c["tz"])
        idx = unknowns(pr["sp"], pr["P"])[2]
        Hr = [[H[i][j] for j in idx] for i in idx]
        ev = eigsy(matrix(Hr), eigvals_only=True)
        return min(ev[i] for i in range(len(idx))), EIG_BAR * max(1.0, max(abs(float(v)) for row in Hr for v in row))


def _chol_solve(L, n, b):
    y = b[:]
    for i in range(n):
        for k in range(i):
            y[i] -= L[i][k] * y[k]
        y[i] /= L[i][i]
    for i in range(n - 1, -1, -1):
        for k in range(i + 1, n):
            y[i] -= L[k][i] * y[k]
        y[i] /= L[i][i]
    return y


def _chol(A, n, sqrt):
    """unblocked LLT, lower: (ok, L); fails at the first non-positive pivot"""
    L = [row[:] for row in A]
    for k in range(n):
        if not L[k][k] > 0:
            return False, L
        L[k][k] = sqrt(L[k][k])
        for i in range(k + 1, n):
            L[i][k] /= L[k][k]
        for j in range(k + 1, n):
            for i in range(j, n):
                L[i][j] -= L[i][k] * L[j][k]
    return True, L


def truth(pr, dps=DPS):
    """the update at 60 digits: the four outputs (z1, t1, lam1, lt1) and the intermediates -- reduced g, H, ev, repaired, shift, x, dxds, wolfe, guard, step0, k, trials (margins).
    `undecidable` holds case (i); decide() adds case (ii)"""
    with mp.workdps(dps):
        c = _inputs(_M, pr)
        g19, H19 = _grad_hess(_M, c, c["z"], c["tz"])
        lo, tn, idx = unknowns(pr["sp"], pr["P"])
        n = len(idx)
        g = [g19[i] for i in idx]
        H = [[H19[i][j] for j in idx] for i in idx]
        evs = eigsy(matrix(H), eigvals_only=True)
        ev = min(evs[i] for i in range(n))
        hmax = max(abs(float(v)) for row in H for v in row)
        ebar = EIG_BAR * max(1.0, hmax)
        repaired = bool(ev <= 0)
        shift = mpf(1) / 100 - ev if ev < 0 else mpf(0)
        Hs = [[H[i][j] + (shift if i == j else 0) for j in range(n)] for i in range(n)]
        ok, L = _chol(Hs, n, mp.sqrt)
        assert ok or ev == 0
        x = [-v for v in _chol_solve(L, n, g)]
        dxds = [-v for v in _chol_solve(L, n, x)]
        out = _search(_M, c, pr, x, idx, lo, tn, g)
        out.update(n=n, lo=lo, tn=tn, idx=idx, g=g, H=H, ev=ev, ebar=ebar, hmax=hmax, repaired=repaired, shift=shift, x=x, dxds=dxds, cx=c["cx"], pr=pr, c=c)
        out["undecidable"], out["why"] = bool(abs(ev) <= ebar), ("eigenvalue" if abs(ev) <= ebar else None)
        return out


def decide(tr, yd):
    """case (ii) of the undecidable pieces: yd is the yardstick's record of the same piece with candidates up to the truth's k.  Marks the truth's record"""
    with mp.workdps(DPS):
        ce = max(abs(float(mpf(yd["e0"]) - tr["e0"])) if math.isfinite(yd["e0"]) else math.inf, U64 * tr["A0"])
        for j, t in enumerate(tr["trials"][:tr["k"] + 1]):
            yen = yd["trials"][j]["en"] if j < len(yd["trials"]) else math.nan
            cn = max(abs(float(mpf(yen) - t["en"])) if math.isfinite(yen) else math.inf, U64 * t["A"])
            if abs(float(t["margin"])) < K * (ce + cn) and not tr["undecidable"]:
                tr["undecidable"], tr["why"] = True, ("armijo", j)
    return tr


def outputs_at(tr, k, dsigma=0):
    """the truth's four outputs had the search accepted 0.8^k, and had the repair's shift been sigma + dsigma"""
    with mp.workdps(DPS):
        x, n = tr["x"], tr["n"]
        if dsigma != 0:
            Hs = [[tr["H"][i][j] + (tr["shift"] + dsigma if i == j else 0) for j in range(n)] for i in range(n)]
            ok, L = _chol(Hs, n, mp.sqrt)
            if not ok:
                return None
            x = [-v for v in _chol_solve(L, n, tr["g"])]
        return _search(_M, tr["c"], tr["pr"], x, tr["idx"], tr["lo"], tr["tn"], tr["g"], force_k=k)


# ---- public: yardstick --------------------------------------------------------------------------------------------------------------------
def yard(pr, fault=None, kmin=0):
    """the update in plain fp64 (own LLT in the natural order, numpy's eigvalsh for the repair).  A fault that ends in a division by zero or a root of a negative number returns NaNs"""
    nan = dict(z1=[math.nan] * 18, t1=math.nan, lam1=[math.nan] * 18, lt1=math.nan, k=-1, trials=[], e0=math.nan, guard=False, repaired=False)
    try:
        c = _inputs(_F, pr)
        g19, H19 = _grad_hess(_F, c, c["z"], c["tz"], fault)
        lo, tn, idx = unknowns(pr["sp"], pr["P"], fault)
        n = len(idx)
        g = [g19[i] for i in idx]
        H = [[H19[i][j] for j in idx] for i in idx]
        ok, L = _chol(H, n, math.sqrt)
        repaired, ev = not ok, None
        if not ok:
            ev = float(np.linalg.eigvalsh(np.array(H))[0])
            if ev < 0:
                for i in range(n):
                    H[i][i] = H[i][i] - ev + (0.0 if fault == "shift001" else 0.01)
            ok, L = _chol(H, n, math.sqrt)
            if not ok:
                return nan
        x = [-v for v in _chol_solve(L, n, g)]
        out = _search(_F, c, pr, x, idx, lo, tn, g, fault, kmin)
        out.update(n=n, repaired=repaired, ev=ev, x=x)
        return out
    except (ZeroDivisionError, OverflowError, ValueError):
        return nan


def state_outputs(st, u, sp):
    """a state's four outputs of one piece, as a record measure() takes"""
    return dict(z1=[float(st["p_slack"][u][a][6 * sp + j]) for a in range(3) for j in range(6)], t1=float(st["t_slack"][u][sp]),
                lam1=[float(st["p_lambda"][u][a][6 * sp + j]) for a in range(3) for j in range(6)], lt1=float(st["t_lambda"][u][sp]))


# ---- the error measure and the bars ---------------------------------------------------------------------------------------------------
def _norm(v):
    return mp.sqrt(sum(x * x for x in v))


def _delta(c, o):
    return [mpf(o["z1"][i]) - c["z"][i] for i in range(18)] + [mpf(o["t1"]) - c["tz"]]


def fit_shift(tr, out, k):
    """a repaired piece: the dsigma, at most the eigenvalue bar in size, at which the truth's shifted solve comes closest to `out` (two Gauss-Newton steps on the one unknown)
    -> (the truth's outputs at sigma + dsigma, dsigma / bar)"""
    c, ebar = tr["c"], mpf(tr["ebar"])
    h = mpf(10) ** -30
    ref, a = outputs_at(tr, k), mpf(0)
    for _ in range(2):
        nxt = outputs_at(tr, k, a + h)
        if nxt is None:
            break
        d0 = _delta(c, ref)
        J = [(p - q) / h for p, q in zip(_delta(c, nxt), d0)]
        d = [p - q for p, q in zip(_delta(c, out), d0)]
        a = a + sum(p * q for p, q in zip(d, J)) / sum(q * q for q in J)
        a = max(-ebar, min(ebar, a))
        new = outputs_at(tr, k, a) if a != 0 else outputs_at(tr, k)
        if new is None:
            break
        ref = new
    return ref, float(a / ebar)


def measure(tr, out, k=None, fit=True):
    """(primal, dual, dual less the one rounding, dsigma / bar): ||delta - delta_truth|| / ||delta_truth|| of one piece, floors as the module docstring states them.  k: against
    the truth's outputs at that back-off count instead of its own"""
    k = tr["k"] if k is None else k
    with mp.workdps(DPS):
        if not all(math.isfinite(v) for v in list(out["z1"]) + [out["t1"], out["lt1"]] + list(out["lam1"])):
            return math.inf, math.inf, math.inf, 0.0
        c = tr["c"]
        z, t, lam, lt, mu = c["z"], c["tz"], c["lam"], c["lt"], c["mu"]
        ref, off = (tr if k == tr["k"] else outputs_at(tr, k)), 0.0
        if tr["repaired"] and fit:
            ref, off = fit_shift(tr, out, k)
        dt = _delta(c, ref)
        num = _norm([a - b for a, b in zip(_delta(c, out), dt)])
        den = max(_norm(dt), U64 * _norm(z + [t]))
        rp = num / den
        lt_ = [ref["lam1"][i] - lam[i] for i in range(18)] + [ref["lt1"] - lt]
        ld = [mpf(out["lam1"][i]) - lam[i] for i in range(18)] + [mpf(out["lt1"]) - lt]
        numd = _norm([a - b for a, b in zip(ld, lt_)])
        rndd = U64 * _norm([mpf(v) for v in out["lam1"]] + [mpf(out["lt1"])])
        mag = [abs(c["cx"][i]) + abs(ref["z1"][i]) for i in range(18)] + [abs(c["pt"]) + abs(ref["t1"])]
        dend = max(_norm(lt_), U64 * mu * _norm(mag))
        return float(rp), float(numd / dend), float(max(mpf(0), numd - rndd) / dend), off


def inside(m, r):
    """a measure() against a class's bars (r_primal, r_dual)"""
    return m[0] <= K * r[0] and m[2] <= K * r[1] and abs(m[3]) < 1.0


def bars(records):
    """(r_primal, r_dual) of a class at a shape: the yardstick's worst measure over its decidable pieces, floored at u.  records: [(truth, yardstick)]"""
    rp, rd = U64, U64
    for tr, yd in records:
        if tr["undecidable"] or yd["k"] != tr["k"]:
            continue
        a, b, _, _ = measure(tr, yd)
        rp, rd = max(rp, a), max(rd, b)
    return rp, rd


# ---- states and cases (seeded; tests/test_slack_ref.py asserts the conditions tests/test_gpu_slack.py relies on) -----------------------------------------
# shape = (tag, mode, P, U): the smallest sizes at which each form exists -- P = 2: both n = 13 mappings and no n = 19; 3: one interior piece; 11: the P6 strides of the slack
# arrays beyond one wave's worth of rows; mode 0: one robot (scn_a, ks = 1e-8); mode 2: one shared piece_time
SHAPES = [("P2", 1, 2, 2), ("P3", 1, 3, 2), ("P5", 1, 5, 2), ("P11", 1, 11, 2), ("single", 0, 3, 1), ("coupled", 2, 3, 4)]
BASE = "P3"
CLASSES = ("real", "dual", "tsmall", "tlarge", "edge", "param")
PARAM_SETS = ((0.01, 0.1), (0.01, 1.0), (0.01, 10.0), (0.1, 0.1), (0.1, 10.0), (10.0, 0.1), (10.0, 1.0), (10.0, 10.0))      # (mu, kt); (0.1, 1) is `real` itself


def shape(tag):
    return next(s for s in SHAPES if s[0] == tag)


def scene_of(scenes, sh):
    _, mode, P, U = sh
    if mode == 0:
        return scenes.scn_a(n_points=4000, pieces=P)
    return dict(scenes.hard(U, 1500, pieces=P), mode=mode)


_STATES = {}


def real_states(scenes, sh, iters=(0, 3, 12)):
    """the port oracle's states after `iters` iterations of the shape's scene at the shipped parameters"""
    if sh[0] not in _STATES:
        from oracle.pyoracle import Engine
        e = Engine("port", scene_of(scenes, sh))
        out, done = {}, 0
        for n in sorted(iters):
            while done < n:
                e.iterate(); done += 1
            out[n] = e.get_state()
        _STATES[sh[0]] = out
    return {k: {n: v.copy() for n, v in st.items()} for k, st in _STATES[sh[0]].items()}


def with_duals(st, seed):
    """seeded non-zero duals of the state's own magnitude (at least 0.1), and p_slack moved by 0.3 sigma"""
    rng = np.random.default_rng([seed, 91])
    out = {k: v.copy() for k, v in st.items()}
    out["p_slack"] = st["p_slack"] + 0.3 * rng.standard_normal(st["p_slack"].shape)
    out["p_lambda"] = rng.standard_normal(st["p_lambda"].shape) * max(np.abs(st["p_lambda"]).max(), 0.1)
    out["t_lambda"] = rng.standard_normal(st["t_lambda"].shape) * max(np.abs(st["t_lambda"]).max(), 0.1)
    return out


def scaled(st, f):
    """t_slack scaled by f (a number or a [U][P] array)"""
    out = {k: v.copy() for k, v in st.items()}
    out["t_slack"] = st["t_slack"] * f
    return out


def edge_scales(pkg, scenes, sh, st, par):
    """per piece the two scales of t_slack, between 0.3 and 1.0 (mode 0: further down), at which the truth's smallest eigenvalue is -10 and +10 eigenvalue bars: the definite / indefinite transition,
    found by bisection (in fp64 down to where fp64 stops telling, then by secant steps on the truth's eigenvalue).  -> (lo[U][P], hi[U][P]): indefinite, definite"""
    ks = scene_of(scenes, sh)["ks"]
    U, P = st["t_slack"].shape
    lo_s, hi_s = np.zeros((U, P)), np.zeros((U, P))
    for u in range(U):
        for sp in range(P):
            pr = problem(pkg, par, ks, P, st, u, sp)
            t0 = pr["tz"]
            idx = unknowns(sp, P)[2]

            def ev64(f):
                c = _inputs(_F, dict(pr, tz=t0 * f))
                H = np.array(_grad_hess(_F, c, c["z"], c["tz"])[1])[np.ix_(idx, idx)]
                return float(np.linalg.eigvalsh(H)[0])

            def evmp(f):
                return min_eig(dict(pr, tz=t0 * f))
            a, b = 0.3, 1.0
            while ev64(a) >= 0 and a > 1e-3:      # (mode 0: ks is 1e5 times smaller, the transition lies below 0.3)
                a, b = 0.3 * a, a
            assert ev64(a) < 0 < ev64(b), (sh[0], u, sp)
            for _ in range(40):
                m = 0.5 * (a + b)
                a, b = (m, b) if ev64(m) < 0 else (a, m)
            f0 = 0.5 * (a + b)
            h = 1e-6
            e0, ebar = evmp(f0)
            slope = float(evmp(f0 + h)[0] - e0) / h          # d ev / d scale > 0
            f0 -= float(e0) / slope
            lo_s[u, sp], hi_s[u, sp] = f0 - 10 * ebar / slope, f0 + 10 * ebar / slope
    return lo_s, hi_s


_CASES = {}


def cases(pkg, scenes, sh, only=None):
    """[(class, name, state, params)] of a shape (only: of one class).  The base shape runs every state; the others the later ones (after an iteration the slack no longer
    equals C x).  tsmall starts from the states after 3 and 12 iterations: at iteration 0 the control net is a straight line, its jerk -- and with it the cross term -- is zero"""
    if only is None:
        return [c for cls in CLASSES for c in cases(pkg, scenes, sh, cls)]
    if (sh[0], only) in _CASES:
        return _CASES[sh[0], only]
    par = dict(scenes.DEFAULT_PARAMS)
    real = real_states(scenes, sh)
    base = sh[0] == BASE
    seed = 100 * sh[2] + 10 * sh[3] + sh[1]
    f1 = 0.03 if sh[1] == 0 else 0.3      # (mode 0, ks = 1e-8: at 0.3 every piece is still definite -- the transition lies between 0.1 and 0.03)
    if only == "real":
        out = [("real", "it%d" % n, real[n], par) for n in ((0, 3, 12) if base else (3, 12))]
    elif only == "dual":
        out = [("dual", "it%d" % n, with_duals(real[n], seed + n), par) for n in ((0, 3, 12) if base else (12,))]
    elif only == "tsmall":
        out = [("tsmall", "it%d*%g" % (n, f), scaled(real[n], f), par) for n, f in (((3, f1), (12, f1), (3, 0.01), (12, 0.01)) if base else ((12, f1), (3, 0.01)))]
    elif only == "tlarge":
        out = [("tlarge", "it%d*5" % n, scaled(real[n], 5.0), par) for n in ((0, 3, 12) if base else (12,))]
    elif only == "edge":
        lo_s, hi_s = edge_scales(pkg, scenes, sh, real[3], par)
        out = [("edge", "it3-", scaled(real[3], lo_s), par), ("edge", "it3+", scaled(real[3], hi_s), par)]
    else:
        assert only == "param"
        out = []
        for i, (mu, kt) in enumerate(PARAM_SETS if base else (PARAM_SETS[2], PARAM_SETS[5])):      # alternately on a real and on a tsmall state: every value of mu and of kt meets both
            st = real[12] if i % 2 == 0 else scaled(real[3], f1)
            out.append(("param", "mu%g,kt%g,%s" % (mu, kt, "real" if i % 2 == 0 else "tsmall"), st, dict(par, mu=mu, kt=kt)))
    _CASES[sh[0], only] = out
    return out


_RECORDS, _BARS = {}, {}


def class_bars(pkg, scenes, sh, cls):
    """(r_primal, r_dual) of a class at a shape, kept"""
    if (sh[0], cls) not in _BARS:
        _BARS[sh[0], cls] = bars([(tr, yd) for c in cases(pkg, scenes, sh, cls) for _, _, tr, yd in case_records(pkg, scenes, sh, c)])
    return _BARS[sh[0], cls]


def case_records(pkg, scenes, sh, name_of_case):
    """[(u, sp, truth, yardstick)] of one case, kept: both test files and every test of a case share them"""
    key = (sh[0],) + name_of_case[:2]
    if key not in _RECORDS:
        cls, name, st, par = name_of_case
        ks = scene_of(scenes, sh)["ks"]
        recs = []
        for u, row in enumerate(problems(pkg, par, ks, sh[2], st)):
            for sp, pr in enumerate(row):
                tr = truth(pr)
                yd = yard(pr, kmin=tr["k"])
                recs.append((u, sp, decide(tr, yd), yd))
        _RECORDS[key] = recs
    return _RECORDS[key]
