"""The x-update's objective of one robot, its per-piece gradient and Hessian and the per-piece PSD repair, three times over -- TEST INFRASTRUCTURE ONLY.

  truth      mpmath at DPS = 60 digits: piece_energy / robot_energy, piece_grad_hess (analytic, before the repair), repair (mpmath.eigsy).
  yardstick  the same formulas in plain fp64, in the natural loop order (per term, from zero): the answer of someone who did not try to be clever.  Its
             distance from the truth says what fp64 costs on these inputs; the device is held to a multiple of it (tests/test_gpu_grad.py).
  faults     six one-line faults that can be planted in the yardstick (FAULTS); tests/test_grad_ref.py shows that each misses the bars.

The objective is restated from the formulas the kernels cite (csrc/kernels_newton.h, csrc/kernels_ls.h; Energy_admm.h:16-170, Gradient_admm.h:67-164, :331-572), not from
the device's order of summation.  Piece sp of a robot owns the control points x[k][a] = net[3 sp + k][a], k < 6, a < 3 (local index 3 k + a) and the flight time t (local
index 18).  With the segment hulls P_i[j] = sum_k basis[sp res + i][j][k] x[k] (i < res, j < 6), the segment weight w_i (the TABLE value (k+1)/res - k/res in fp64: an input,
as seg_weight forms it) and b_w(d) = -w (d - m)^2 ln(d/m) for 0 < d < m, 0 for d >= m, +inf for d <= 0 (m = margin):

  E_sp(x, t) = lambda sum_i [ sum_{planes (n, o) of segment i} sum_j b_w(n . P_i[j] + o)
                              + sum_{b<5} b_w(vel_limit - 5 |P_i[b+1] - P_i[b]| / (w_i t))
                              + sum_{b<4} b_w(acc_limit - 20 |P_i[b+2] - 2 P_i[b+1] + P_i[b]| / (w_i t)^2) ]
               + mu/2 |C x - z|^2 + Lambda . (C x - z) + mu/2 (t - t_z)^2 + lambda_t (t - t_z),          C = convert[sp], z / Lambda / t_z / lambda_t the piece's slack and dual blocks

and E = sum_sp E_sp.  The derivatives are formed by the chain rule on d(x, t) = L - s |D| with s = c / t^p ((c, p) = (5/w, 1), (20/w^2, 2)), D = sum_a wv[a] x[a]:
b'' grad d grad d^T + b' Hess d, every term written out in _piece_gh.  tests/test_grad_ref.py compares them with central differences of piece_energy at 80 digits: the block
documented at Gradient_admm.h IS the exact Hessian of this function (no Gauss-Newton shortcut anywhere; the finite differences agree to 1e-20 of the magnitude sum in
every entry), so nothing had to be followed against the exact derivative.

Magnitude sums.  Every entry comes with A = the sum of the absolute values of the terms that make it up, at the granularity of the formulas above: one term per (plane,
hull point), per record and per sub-term of b' = -w (2 (d-m) ln(d/m) + (d-m)^2/d) and b'' = -w (2 ln(d/m) + 4 (d-m)/d - (d-m)^2/d^2); a consensus term mu C^T (C x - z)
counts mu |C|^T (|C| |x| + |z|), and so on (a difference enters with the magnitude sum of ITS terms).  A is computed in fp64 -- it only scales a bar.
The one place that needs care: fl(d/m) = (d/m)(1 + delta), |delta| <= u = 2^-53, moves ln(d/m) by delta ABSOLUTELY, however small the logarithm is.  For d within a few ulps of m
the term 2 w ln(d/m) of b'' (coefficient 2 w) therefore carries an error of 2 w u that does not shrink with the term; so |ln(d/m)| enters A as max(|ln(d/m)|, u) wherever it
appears: the term's contribution is floored at w u times its coefficient.

Bars (see bars()): r_class = the yardstick's worst |yardstick - truth| / A over a class of inputs at one shape, floored at u; a value is accepted within K r_class A.
"""
import math

import numpy as np
from mpmath import mp, mpf, eigsy, matrix

DPS = 60
U64 = 2.0 ** -53
FAULTS = ("acc_tsign", "bit63", "lastplane", "e2term", "mu1818", "lam_z_piece")
EIG_BAR = 1e-12      # the project's eigenvalue bar (test_device_llt_and_min_eigenvalue): 1e-12 max(1, |H|_max)


class _F:      # the yardstick's arithmetic
    num = float
    log = staticmethod(math.log)
    sqrt = staticmethod(math.sqrt)
    inf = math.inf


class _M:      # the truth's
    num = staticmethod(mpf)
    log = staticmethod(mp.log)
    sqrt = staticmethod(mp.sqrt)
    inf = mp.inf


def seg_weights(res):
    return [(k + 1) / float(res) - k / float(res) for k in range(res)]


def problem(pkg, params, P, state, u, planes_u):
    """one robot's inputs: params (the Solver's dict), its state and its plane lists (planes_u: per segment an [n][4] array)"""
    res = params["res"]
    conv, _, basis, _ = pkg.host_tables(P, res)
    return dict(res=res, P=P, lam=params["lam"], mu=params["mu"], margin=params["margin"], vel_limit=params["vel_limit"], acc_limit=params["acc_limit"],
                basis=basis, convert=conv, wseg=seg_weights(res), spline=np.array(state["spline"][u]), p_slack=np.array(state["p_slack"][u]),
                p_lambda=np.array(state["p_lambda"][u]), t_slack=np.array(state["t_slack"][u]), t_lambda=np.array(state["t_lambda"][u]),
                t=float(state["piece_time"][u]), planes=[np.asarray(p, dtype=np.float64).reshape(-1, 4) for p in planes_u])


def split_planes(counts, planes):
    """(counts[U][S], planes[sum][4]) as stage_planes / get_planes return them -> [u][segment] -> [n][4]"""
    planes = np.asarray(planes).reshape(-1, 4)
    out, w = [], 0
    for cu in np.asarray(counts):
        row = []
        for n in cu:
            row.append(planes[w:w + n]); w += n
        out.append(row)
    return out


# ---- the formulas, once, over an arithmetic ---------------------------------------------------------------------------------------------
def _x0(ar, pr, sp):
    return [[ar.num(pr["spline"][a][3 * sp + k]) for a in range(3)] for k in range(6)]


def _hull(ar, B, x):
    P = []
    for j in range(6):
        row = []
        for a in range(3):
            acc = ar.num(0)
            for k in range(6):
                acc += B[j][k] * x[k][a]
            row.append(acc)
        P.append(row)
    return P


def _tab(ar, M):
    return [[ar.num(v) for v in row] for row in M]


def _basis(ar, pr, tr):
    """segment tr's basis in the arithmetic (the conversions are exact; kept with the problem: an energy is evaluated hundreds of times by the finite differences)"""
    key = ("basis", ar.__name__, tr)
    if key not in pr:
        pr[key] = _tab(ar, pr["basis"][tr])
    return pr[key]


def _planes(ar, pr, tr):
    key = ("planes", ar.__name__, tr)
    if key not in pr:
        pr[key] = _tab(ar, pr["planes"][tr])
    return pr[key]


def _logm(L):
    return max(abs(float(L)), U64)


def _records(ar, pr, tr, P, w, t, want_wv=True):
    """the nine limit records of segment tr: (index b, d, L, s, p, r, D, wv) with d = L - s r, s = c / t^p, r = |D|, D = sum_a wv[a] x[a] (wv: differences of basis rows)"""
    B = _basis(ar, pr, tr)
    for b in range(9):
        if b < 5:
            D = [P[b + 1][a] - P[b][a] for a in range(3)]
            wv = [B[b + 1][k] - B[b][k] for k in range(6)] if want_wv else None
            L, s, p = ar.num(pr["vel_limit"]), 5 / (w * t), 1
        else:
            j = b - 5
            D = [P[j + 2][a] - 2 * P[j + 1][a] + P[j][a] for a in range(3)]
            wv = [B[j + 2][k] - 2 * B[j + 1][k] + B[j][k] for k in range(6)] if want_wv else None
            L, s, p = ar.num(pr["acc_limit"]), 20 / ((w * t) * (w * t)), 2
        r = ar.sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2])
        yield b, L - s * r, L, s, p, r, D, wv


def _piece_energy(ar, pr, sp, x=None, t=None, fault=None, mags=False):
    """E_sp (and, mags: its magnitude sum, fp64 arithmetic only)"""
    res, m = pr["res"], ar.num(pr["margin"])
    x = _x0(ar, pr, sp) if x is None else x
    t = ar.num(pr["t"]) if t is None else t
    bad, eb, A = False, ar.num(0), 0.0
    lam, mu = ar.num(pr["lam"]), ar.num(pr["mu"])

    def bar(w, d):
        nonlocal bad, eb, A
        if d <= 0:
            bad = True
        elif d < m:
            L = ar.log(d / m)
            eb += -w * (d - m) * (d - m) * L
            if mags:
                A += float(lam) * float(w) * float(d - m) ** 2 * _logm(L)
    for i in range(res):
        tr = sp * res + i
        w = ar.num(pr["wseg"][i])
        P = _hull(ar, _basis(ar, pr, tr), x)
        pls = _planes(ar, pr, tr)
        if fault == "lastplane" and len(pls) % 4:
            pls = pls[:-1]
        for pl in pls:
            n0, n1, n2, off = pl
            for j in range(6):
                bar(w, P[j][0] * n0 + P[j][1] * n1 + P[j][2] * n2 + off)
        for b, d, *_ in _records(ar, pr, tr, P, w, t, False):
            if fault == "bit63" and i * 9 + b == 63:
                continue
            bar(w, d)
    e = lam * eb
    C = _tab(ar, pr["convert"][sp])
    zp = (sp + 1) % pr["P"] if fault == "lam_z_piece" else sp
    for a in range(3):
        for j in range(6):
            cx, acx = ar.num(0), 0.0
            for k in range(6):
                cx += C[j][k] * x[k][a]
                acx += abs(float(C[j][k]) * float(x[k][a]))
            z, z2, La = ar.num(pr["p_slack"][a][sp * 6 + j]), ar.num(pr["p_slack"][a][zp * 6 + j]), ar.num(pr["p_lambda"][a][sp * 6 + j])
            dl = cx - z
            e += mu / 2 * (dl * dl)
            e += La * (cx - z2)
            if mags:
                ad = acx + abs(float(z))
                A += float(mu) * abs(float(dl)) * ad + abs(float(La)) * ad
    tz, lt = ar.num(pr["t_slack"][sp]), ar.num(pr["t_lambda"][sp])
    dt = t - tz
    e += mu / 2 * (dt * dt)
    e += lt * dt
    if mags:
        at = abs(float(t)) + abs(float(tz))
        A += float(mu) * abs(float(dt)) * at + abs(float(lt)) * at
    e = ar.inf if bad else e
    return (e, A) if mags else e


def _bd(ar, w, d, m, fault=None):
    """b', b'' and their magnitude sums (floats)"""
    L, q = ar.log(d / m), d - m
    e1 = -w * (2 * q * L + q * q / d)
    e2 = -w * (2 * L + (0 if fault == "e2term" else 4 * q / d) - q * q / (d * d))
    fw, fq, fd, la = float(w), abs(float(q)), float(d), _logm(L)
    return e1, e2, fw * (2 * fq * la + fq * fq / fd), fw * (2 * la + 4 * fq / fd + fq * fq / (fd * fd))


def _apply(g, H, c, N, v, tv=None):
    """a term whose x-dependence runs through the 6-vector c: H[(a,q),(a',q')] += c_a c_a' N[q][q'], g[(a,q)] += c_a v[q], H[(a,q),18] += c_a tv[q] (lower triangle)"""
    for a in range(6):
        ca = c[a]
        for q in range(3):
            i = 3 * a + q
            g[i] += ca * v[q]
            if tv is not None:
                H[18][i] += ca * tv[q]
            for a2 in range(a + 1):
                cc = ca * c[a2]
                for q2 in range(3 if a2 < a else q + 1):
                    H[i][3 * a2 + q2] += cc * N[q][q2]


def _piece_gh(ar, pr, sp, fault=None, mags=False, group=False):
    """(g[19], H[19][19]) of E_sp before the repair [+ (Ag, AH), mags].  group: the planes of a (segment, hull point) are summed into one 3x3 matrix and one 3-vector
    before they are spread over the entries (the truth only: at 60 digits the order of summation is immaterial, and it is ~50 times fewer operations)"""
    res, m, t = pr["res"], ar.num(pr["margin"]), ar.num(pr["t"])
    lam, mu = ar.num(pr["lam"]), ar.num(pr["mu"])
    x = _x0(ar, pr, sp)
    z0 = ar.num(0)
    g, H = [z0] * 19, [[z0] * 19 for _ in range(19)]          # barrier terms, before lambda
    Ag, AH = [0.0] * 19, [[0.0] * 19 for _ in range(19)]
    for i in range(res):
        tr = sp * res + i
        w = ar.num(pr["wseg"][i])
        B = _basis(ar, pr, tr)
        P = _hull(ar, B, x)
        pls = _planes(ar, pr, tr)
        if fault == "lastplane" and len(pls) % 4:
            pls = pls[:-1]
        for j in range(6):
            c = B[j]
            ca = [abs(float(v)) for v in c]
            N, v = [[z0] * 3 for _ in range(3)], [z0] * 3
            AN, Av = [[0.0] * 3 for _ in range(3)], [0.0] * 3
            for pl in pls:
                n = pl[:3]
                d = P[j][0] * n[0] + P[j][1] * n[1] + P[j][2] * n[2] + pl[3]
                if not d < m:
                    continue
                e1, e2, a1, a2 = _bd(ar, w, d, m, fault)
                N1 = [[e2 * (n[q] * n[q2]) for q2 in range(3)] for q in range(3)]
                v1 = [e1 * n[q] for q in range(3)]
                if group:
                    for q in range(3):
                        v[q] += v1[q]
                        for q2 in range(3):
                            N[q][q2] += N1[q][q2]
                else:
                    _apply(g, H, c, N1, v1)
                if mags:
                    fn = [abs(float(y)) for y in n]
                    for q in range(3):
                        Av[q] += a1 * fn[q]
                        for q2 in range(3):
                            AN[q][q2] += a2 * fn[q] * fn[q2]
            if group:
                _apply(g, H, c, N, v)
            if mags:
                _apply(Ag, AH, ca, AN, Av)
        for b, d, L, s, p, r, D, wv in _records(ar, pr, tr, P, w, t):
            if not d < m or (fault == "bit63" and i * 9 + b == 63):
                continue
            e1, e2, a1, a2 = _bd(ar, w, d, m, fault)
            nh = [D[q] / r for q in range(3)]
            dt1 = p * s * r / t                       # dd/dt
            dt2 = -p * (p + 1) * s * r / (t * t)      # d2d/dt2
            # dd/dx = -s wv (x) nh;  d2d/dx2 = -s wv wv^T (x) (I - nh nh^T) / r;  d2d/dxdt = (p s / t) wv (x) nh
            N = [[e2 * (s * s) * (nh[q] * nh[q2]) + e1 * (-s) * (((1 if q == q2 else 0) - nh[q] * nh[q2]) / r) for q2 in range(3)] for q in range(3)]
            v = [e1 * (-s) * nh[q] for q in range(3)]
            tv = [e2 * dt1 * (-s) * nh[q] + e1 * (p * s / t) * nh[q] for q in range(3)]
            if fault == "acc_tsign" and b >= 5:
                tv = [-y for y in tv]
            _apply(g, H, wv, N, v, tv)
            g[18] += e1 * dt1
            H[18][18] += e2 * dt1 * dt1 + e1 * dt2
            if mags:
                fs, fr, fn, ft, f1, f2 = float(s), float(r), [abs(float(y)) for y in nh], float(t), abs(float(dt1)), abs(float(dt2))
                AN = [[a2 * fs * fs * fn[q] * fn[q2] + a1 * fs * ((1 if q == q2 else 0) + fn[q] * fn[q2]) / fr for q2 in range(3)] for q in range(3)]
                Av = [a1 * fs * fn[q] for q in range(3)]
                Atv = [a2 * f1 * fs * fn[q] + a1 * (p * fs / ft) * fn[q] for q in range(3)]
                _apply(Ag, AH, [abs(float(y)) for y in wv], AN, Av, Atv)
                Ag[18] += a1 * f1
                AH[18][18] += a2 * f1 * f1 + a1 * f2
    C = _tab(ar, pr["convert"][sp])
    go, Ho = [lam * y for y in g], [[lam * y for y in row] for row in H]
    fl, fm = float(lam), float(mu)
    Ag, AH = [fl * y for y in Ag], [[fl * y for y in row] for row in AH]
    for a in range(6):
        for q in range(3):
            i = 3 * a + q
            acc, acl, aacc, aacl = ar.num(0), ar.num(0), 0.0, 0.0
            for j in range(6):
                cx, acx = ar.num(0), 0.0
                for k in range(6):
                    cx += C[j][k] * x[k][q]
                    acx += abs(float(C[j][k]) * float(x[k][q]))
                z, La = ar.num(pr["p_slack"][q][sp * 6 + j]), ar.num(pr["p_lambda"][q][sp * 6 + j])
                acc += C[j][a] * (cx - z); acl += C[j][a] * La
                aacc += abs(float(C[j][a])) * (acx + abs(float(z))); aacl += abs(float(C[j][a]) * float(La))
            go[i] += mu * acc + acl
            Ag[i] += fm * aacc + aacl
            for a2 in range(a + 1):
                k2 = 3 * a2 + q
                mab, amab = ar.num(0), 0.0
                for j in range(6):
                    mab += C[j][a] * C[j][a2]; amab += abs(float(C[j][a]) * float(C[j][a2]))
                Ho[i][k2] += mu * mab
                AH[i][k2] += fm * amab
    tz, lt = ar.num(pr["t_slack"][sp]), ar.num(pr["t_lambda"][sp])
    go[18] += mu * (t - tz) + lt
    Ag[18] += fm * (abs(float(t)) + abs(float(tz))) + abs(float(lt))
    if fault != "mu1818":
        Ho[18][18] += mu
    AH[18][18] += fm
    for i in range(19):
        for k in range(i):
            Ho[k][i] = Ho[i][k]; AH[k][i] = AH[i][k]
    return (go, Ho, Ag, AH) if mags else (go, Ho)


# ---- public: truth --------------------------------------------------------------------------------------------------------------------
def piece_energy(pr, sp, x18=None, t=None, dps=DPS):
    """the truth's E_sp (mpf; +inf where a hull point or a limit has d <= 0); x18 / t: evaluate there instead of at the state (mpf: [6][3] control points, time)"""
    with mp.workdps(dps):
        return _piece_energy(_M, pr, sp, x18, t)


def robot_energy(pr, dps=DPS):
    with mp.workdps(dps):
        e = mpf(0)
        for sp in range(pr["P"]):
            e += _piece_energy(_M, pr, sp)
        return e


def piece_grad_hess(pr, sp, dps=DPS):
    """(g, H, Ag, AH): the analytic gradient (19) and Hessian (19 x 19) in mp before the repair, and the fp64 magnitude sums of their entries"""
    with mp.workdps(dps):
        g, H = _piece_gh(_M, pr, sp, group=True)
    _, _, Ag, AH = _piece_gh(_F, pr, sp, mags=True)
    return g, H, np.array(Ag), np.array(AH)


def repair(H, dps=DPS):
    """(lambda_min, repaired?, shift, undecidable?): the block is repaired iff it is not positive definite, by H + (-lambda_min + 0.01) I; blocks whose lambda_min lies
    within EIG_BAR max(1, |H|_max) of 0 are undecidable in fp64"""
    with mp.workdps(dps):
        ev = eigsy(matrix(H), eigvals_only=True)
        lmin = min(ev[i] for i in range(19))
        hmax = max(abs(float(H[i][k])) for i in range(19) for k in range(19))
        return lmin, bool(lmin <= 0), 0.01 - lmin, bool(abs(lmin) <= EIG_BAR * max(1.0, hmax))


def fd_grad_hess(pr, sp, h=mpf("1e-25"), dps=80):
    """central differences of piece_energy: (g[19], H[19][19]) as mpf"""
    with mp.workdps(dps):
        x0, t0 = _x0(_M, pr, sp), mpf(pr["t"])

        def E(moves):
            x = [row[:] for row in x0]; t = t0
            for i, s in moves:
                if i == 18:
                    t = t + s * h
                else:
                    x[i // 3][i % 3] = x[i // 3][i % 3] + s * h
            return _piece_energy(_M, pr, sp, x, t)
        e0 = E(())
        g, H = [None] * 19, [[None] * 19 for _ in range(19)]
        ep = [E(((i, 1),)) for i in range(19)]; em = [E(((i, -1),)) for i in range(19)]
        for i in range(19):
            g[i] = (ep[i] - em[i]) / (2 * h)
            H[i][i] = (ep[i] - 2 * e0 + em[i]) / (h * h)
            for k in range(i):
                H[i][k] = H[k][i] = (E(((i, 1), (k, 1))) - E(((i, 1), (k, -1))) - E(((i, -1), (k, 1))) + E(((i, -1), (k, -1)))) / (4 * h * h)
        return g, H


# ---- public: yardstick ------------------------------------------------------------------------------------------------------------------
def yard_grad_hess(pr, sp, fault=None):
    g, H = _piece_gh(_F, pr, sp, fault=fault)
    return np.array(g), np.array(H)


def yard_energy(pr, fault=None):
    """(E, A) of the robot in fp64: the pieces' energies added in piece order"""
    e, A = 0.0, 0.0
    for sp in range(pr["P"]):
        e1, a1 = _piece_energy(_F, pr, sp, fault=fault, mags=True)
        e += e1; A += a1
    return e, A


def active_records(pr, sp):
    """the 9 res activity bits of piece sp's limit records, as k_grad's mask holds them (bit 9 i + b), and whether any limit is violated"""
    bits, bad = [], False
    x, t = _x0(_F, pr, sp), pr["t"]
    for i in range(pr["res"]):
        tr = sp * pr["res"] + i
        P = _hull(_F, _basis(_F, pr, tr), x)
        for b, d, *_ in _records(_F, pr, tr, P, pr["wseg"][i], t, False):
            bits.append(d < pr["margin"]); bad |= d <= 0
    return np.array(bits), bad


# ---- truth of a whole fleet, and the bars --------------------------------------------------------------------------------------------
def fleet_truth(probs):
    """per robot and piece the truth and the yardstick: dict(g, H, Ag, AH (before the repair), lmin, repaired, shift, undecidable, yg, yH), and per robot (E, AE, yE)"""
    blocks, ener = [], []
    for pr in probs:
        row = []
        for sp in range(pr["P"]):
            g, H, Ag, AH = piece_grad_hess(pr, sp)
            lmin, rep, shift, und = repair(H)
            yg, yH = yard_grad_hess(pr, sp)
            row.append(dict(g=g, H=H, Ag=Ag, AH=AH, lmin=lmin, repaired=rep, shift=shift, undecidable=und, yg=yg, yH=yH))
        blocks.append(row)
        E = robot_energy(pr)
        yE, AE = yard_energy(pr)
        ener.append((E, AE, yE))
    return blocks, ener


def block_ratio(b, g, H, r=1.0, diag=True):
    """worst |value - truth| / (r A) over the gradient and the Hessian of one block (g[19], H[19][19] fp64; diag = False: off-diagonal entries only)"""
    worst = 0.0
    with mp.workdps(DPS):
        for i in range(19):
            if b["Ag"][i] > 0 or g[i] != 0:
                worst = max(worst, float(abs(mpf(float(g[i])) - b["g"][i])) / (r * b["Ag"][i]) if b["Ag"][i] > 0 else math.inf)
            for k in range(19):
                if i == k and not diag:
                    continue
                if b["AH"][i][k] > 0 or H[i][k] != 0:
                    worst = max(worst, float(abs(mpf(float(H[i][k])) - b["H"][i][k])) / (r * b["AH"][i][k]) if b["AH"][i][k] > 0 else math.inf)
    return worst


def energy_ratio(en, e, r=1.0):
    E, AE, _ = en
    with mp.workdps(DPS):
        if E == mp.inf or not math.isfinite(e):
            return 0.0 if (E == mp.inf and e == math.inf) else math.inf
        return float(abs(mpf(float(e)) - E)) / (r * AE)


def bars(blocks, ener):
    """(r_blocks, r_energy): the yardstick's worst distance from the truth relative to the magnitude sums over a class at one shape, floored at u"""
    rb = max([U64] + [block_ratio(b, b["yg"], b["yH"]) for row in blocks for b in row])
    re = max([U64] + [energy_ratio(en, en[2]) for en in ener if en[0] != mp.inf])
    return rb, re


# ---- the states and plane lists of tests/test_gpu_grad.py (seeded; conditions asserted in tests/test_grad_ref.py) ------------------------------------
def scene_of(scenes, mode, P, U):
    if mode == 0:
        return scenes.scn_a(n_points=4000, pieces=P)
    return dict(scenes.hard(U, 3000, pieces=P), mode=mode)


_STATES = {}


def real_states(scenes, mode, P, U, params, iters=(0, 3, 12)):
    """(a): the oracle's states after `iters` iterations of the scene at `params`"""
    key = (mode, P, U, tuple(sorted(params.items())), iters)
    if key not in _STATES:
        from oracle.pyoracle import Engine
        e = Engine("port", scene_of(scenes, mode, P, U), params)
        out, done = {}, 0
        for n in sorted(iters):
            while done < n:
                e.iterate(); done += 1
            out[n] = e.get_state()
        _STATES[key] = out
    return {k: {n: v.copy() for n, v in st.items()} for k, st in _STATES[key].items()}


def vary(st, seed, coupled=False):
    """(b): per-robot flight times (longer only: no limit gets closer) and seeded slack / dual blocks of the state's own magnitude"""
    rng = np.random.default_rng([seed, 77])
    out = {k: v.copy() for k, v in st.items()}
    U, P = out["t_slack"].shape
    if not coupled:
        out["piece_time"] = st["piece_time"] * (1.0 + 0.2 * rng.uniform(size=U))
    out["t_slack"] = out["piece_time"][:, None] * (1.0 + 0.05 * rng.normal(size=(U, P)))
    out["t_lambda"] = rng.normal(size=(U, P)) * max(np.abs(st["t_lambda"]).max(), 0.1)
    out["p_lambda"] = rng.normal(size=st["p_lambda"].shape) * max(np.abs(st["p_lambda"]).max(), 0.1)
    return out


def record_values(pkg, params, P, st):
    """(speeds, accelerations) of every velocity / acceleration record of the fleet at the state: what the limits are compared with"""
    v, a = [], []
    none = [np.zeros((0, 4))] * (P * params["res"])
    for u in range(st["spline"].shape[0]):
        pr = problem(pkg, dict(params, vel_limit=0.0, acc_limit=0.0), P, st, u, none)
        for sp in range(P):
            x = _x0(_F, pr, sp)
            for i in range(pr["res"]):
                tr = sp * pr["res"] + i
                for b, d, *_ in _records(_F, pr, tr, _hull(_F, _basis(_F, pr, tr), x), pr["wseg"][i], pr["t"], False):
                    (v if b < 5 else a).append(-d)
    return np.array(v), np.array(a)


def binding_state(pkg, params, P, st, seed, sigma=0.02, peak=4.0, eps=0.02):
    """(c): the state with a seeded wobble on the free control points (speeds and accelerations then differ from segment to segment), flown at the pace that puts
    the fleet's peak speed at `peak` margins, and the limits eps margins above ITS peak speed and peak acceleration: every record within a margin of the peak is active,
    the highest ones sit close to the limit (where the time column makes blocks indefinite), none is violated.  -> (state, params)"""
    rng = np.random.default_rng([seed, 78])
    out = {k: v.copy() for k, v in st.items()}
    T = out["spline"].shape[2]
    out["spline"][:, :, 2:T - 2] += sigma * rng.normal(size=out["spline"][:, :, 2:T - 2].shape)
    m = params["margin"]
    v, a = record_values(pkg, params, P, out)
    f = v.max() / (peak * m) if peak else 1.0      # peak = None: the state's own pace
    out["piece_time"] = out["piece_time"] * f; out["t_slack"] = out["t_slack"] * f
    v, a = record_values(pkg, params, P, out)
    vl, al = float(v.max()) + eps * m, float(a.max()) + eps * m
    return out, dict(params, vel_limit=vl, acc_limit=al)


def edge_time(pkg, params, P, st, u):
    """(d): the flight time of robot u at which its tightest limit record has d = 0 exactly (in real arithmetic): below it the energy is +inf"""
    v, a = record_values(pkg, params, P, {k: val[u:u + 1] for k, val in st.items()})
    t = float(st["piece_time"][u])
    return t * max(v.max() / params["vel_limit"], math.sqrt(a.max() / params["acc_limit"]))


SYN_COUNTS = (0, 1, 3, 4, 5, 17, 64, 65, 100)


def synthetic_counts(U, P, res, big=0):
    """per-(robot, segment) plane counts from SYN_COUNTS.  Robot 0 (res >= 8): piece 0 carries 4 x 17 + ... (its total crosses 64: two batches at the default capacity),
    piece 1 a 64 / 65 pair, a 100 and a 0 between non-zero counts; its remaining pieces and the other robots cycle through the small counts, robot 1 below 43 planes in
    total (the energy's four-pass loop needs 6 M / 64 >= 4).  big > 0: robot 0's total is raised beyond it with counts of 17 (the line search's LDS plane capacity)"""
    S = P * res
    c = np.zeros((U, S), dtype=np.int32)
    heavy = [17, 17, 17, 17, 5, 0, 3, 1, 64, 65, 4, 0, 1, 3, 5, 100]
    small = [1, 0, 3, 4, 5, 0, 17, 0]
    for s in range(S):
        c[0, s] = heavy[s] if s < len(heavy) and res >= 8 else small[(s + 1) % 8]
    if res < 8:     # the same features, a piece being shorter: one long segment per piece
        for s, n in zip(range(0, S, max(1, res)), (65, 100, 64)):
            c[0, s] = n
    for u in range(1, U):
        for s in range(S):
            c[u, s] = (3, 0, 1, 0, 4, 0, 0, 5)[(s + u) % 8] if s < 24 else 0
    s = S - 1
    while big and c[0].sum() <= big:
        c[0, s] = 17; s -= 1
    return c


def synthetic_planes(pkg, params, P, st, counts, seed, behind=None):
    """unit normals through points near the hulls: every plane touches the barrier's range at its segment's lowest hull point along the normal (d = rho m there,
    rho in [0.2, 0.9]); the other five points lie further out, some beyond the range.  behind = (u, segment, d): that segment's first plane gets d at its lowest point"""
    rng = np.random.default_rng([seed, 79])
    res, m = params["res"], params["margin"]
    _, _, basis, _ = pkg.host_tables(P, res)
    out = []
    for u in range(counts.shape[0]):
        for tr in range(counts.shape[1]):
            x = st["spline"][u][:, 3 * (tr // res):3 * (tr // res) + 6].T       # [6][3]
            hull = basis[tr] @ x
            for k in range(counts[u, tr]):
                n = rng.normal(size=3); n /= np.linalg.norm(n)
                d = m * rng.uniform(0.2, 0.9)
                if behind is not None and behind[:2] == (u, tr) and k == 0:
                    d = behind[2]
                out.append([n[0], n[1], n[2], d - float(np.min(hull @ n))])
    return np.array(out).reshape(-1, 4)


# ---- the cases: shapes x classes (tests/test_gpu_grad.py runs them on the device; tests/test_grad_ref.py asserts the conditions they rely on) ------------------------
# shape = (tag, mode, P, res, parameter set).  res: 7 = 63 records, one mask word; 8 = the first 9-bit group across bits 63/64; 15, 16 = the third word and the folded
# launch's second basis register.  P: 2 = every piece is a first or a last one; 11 = the energy's non-affine layout with four groups.
SHAPES = [("res%d" % r, 1, 3, r, None) for r in (1, 7, 8, 9, 15, 16)] + [("P%d" % p, 1, p, 8, None) for p in (2, 5, 11)] + \
         [("single", 0, 3, 8, None), ("coupled", 2, 3, 8, None), ("setA", 1, 3, 8, "A")]
BASE = "res8"
CLASSES_BASE = ("a0", "a3", "a12", "b0", "b3", "b12", "c_dense", "c_tight", "syn")
CLASSES = ("a12", "b12", "c_dense", "c_tight", "syn")     # every other shape: a real state with non-zero slack and duals (after 12 iterations every scene carries planes), (b), both (c) states, the synthetic lists


def shape(tag):
    return next(s for s in SHAPES if s[0] == tag)


def shape_params(scenes, sh):
    from test_oracle_params import PARAM_SETS
    p = dict(scenes.DEFAULT_PARAMS)
    if sh[4]:
        p.update(PARAM_SETS[sh[4]])
    p["res"] = sh[3]
    return p


def fleet(sh):
    return 1 if sh[1] == 0 else 2


def case(pkg, scenes, sh, cls):
    """-> (state, params, plane lists: "own" = the lists the stages build for the state, "none" = empty lists, "syn" = synthetic_planes over synthetic_counts)"""
    _, mode, P, res, _ = sh
    U, par = fleet(sh), shape_params(scenes, sh)
    real = real_states(scenes, mode, P, U, par)
    seed = 1000 * P + 10 * res + mode
    if cls[0] == "a":
        return real[int(cls[1:])], par, "own"
    if cls[0] == "b":
        return vary(real[int(cls[1:])], seed, coupled=mode == 2), par, "own"
    if cls == "c_dense":      # every record within a margin of the peak: every mask word full
        st, cp = binding_state(pkg, par, P, real[3], seed, peak=1.5)
        return st, cp, "none"
    if cls == "c_tight":      # the state's own pace: few records, close to the limit -- idle segments between active ones, indefinite blocks
        st, cp = binding_state(pkg, par, P, real[3], seed, peak=None)
        return st, cp, "none"
    assert cls == "syn"
    return real[3], par, "syn"


def problems(pkg, par, P, st, counts, planes):
    lists = split_planes(counts, planes)
    return [problem(pkg, par, P, st, u, lists[u]) for u in range(len(lists))]
