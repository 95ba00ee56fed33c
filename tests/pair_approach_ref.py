"""Reference values for tj_pair_approach that share no code with csrc/kernels_pair_approach.h (plain module: no fixtures, no tests).

  pair_rows           the Python restatement of include/trajadmm.h's definition, compared with == by tests/test_gpu_pair_approach.py.  The windows, their lo
                      (with its certificate), hi and time are closest_ref._Eval's; the seeds are closest_ref.seeds_of's, FILTERED TO ONE PARTNER; the search
                      is closest_ref.search's loop with "the robot's windows" replaced by "the pair's windows":
                        listed    (u, q) is listed iff one of its seeds has lo < range or hi < range; an unlisted pair has no row
                        seeds     best = the pair's smallest hi < range in the order (hi, segment, partner, time); live = {lo < range and lo < best.hi}
                        round d   every live window is halved (cm == ca or cm == cb: terminal); children from the raw hulls; best over (best, children);
                                  live = children and terminals with lo < best.hi, against the round's FINAL best
                        bracket   lo = min(best.hi, min lo over live), hi = best.hi
                        stop      hi - lo <= tol | live empty | every live window terminal | d == max_depth | more than max_windows live IN THIS PAIR
                                  (TRUNCATED: the record of the last completed round; `windows` counts the overflowing round too)
                      Rows are sorted by (robot, partner).
  merge_symmetric     what Solver.pair_approach(symmetric=True) does, restated with plain loops over dicts.
  default_tolerance   the measured TJ_PAIR_TOL and TJ_PAIR_FRONTIER (the manner of closest_ref.default_tolerance), and the listed pairs per state.
The truth, the slack and the constructed states are audit_timed_ref's."""
import math

import numpy as np

import audit_ref as R
import audit_timed_ref as T
import closest_ref as K

CONTACT, CLEAR, CONVERGED, TRUNCATED = 1, 2, 4, 8
MAX_DEPTH, MAX_WINDOWS = 40, 4096
FIELDS = ("lo", "hi", "time", "robot", "partner", "segment", "depth", "flags", "windows")


def seeds_by_partner(ev, u, rng):
    """{q: ([window], [(lo, hi, time)])} of robot u: closest_ref.seeds_of's windows, evaluated once and filed under their partner"""
    seeds = K.seeds_of(ev, u, rng)
    out = {}
    for w, v in zip(seeds, ev(u, seeds)):
        ws, vs = out.setdefault(w[1], ([], []))
        ws.append(w); vs.append(v)
    return out


def search(ev, u, seeds, vals, rng, tol, max_depth, max_windows, trace=None):
    """the record of one directed pair from its seeds, or None if the pair is not listed; trace receives (depth, lo, hi, size of the live set) per completed round"""
    if not any(lo < rng or hi < rng for lo, hi, _ in vals):
        return None
    NONE = (rng, math.inf, math.inf, math.inf)
    windows = len(seeds)
    best = min([(hi, w[0], w[1], t) for w, (lo, hi, t) in zip(seeds, vals) if hi < rng] + [NONE])
    live = [(w, lo, False) for w, (lo, hi, t) in zip(seeds, vals) if lo < rng and lo < best[0]]
    rec = dict(best=best, lo=min([best[0]] + [l for _, l, _ in live]), depth=0)
    truncated = len(live) > max_windows
    if trace is not None:
        trace.append((0, rec["lo"], best[0], len(live)))
    d = 0
    while not truncated:
        if rec["best"][0] - rec["lo"] <= tol or not live or all(t for _, _, t in live) or d == max_depth:
            break
        kids, terms = [], []
        for (tr, q, j, ca, cb), lo, term in live:
            cm = 0.5 * (ca + cb)
            if term or cm == ca or cm == cb:
                terms.append(((tr, q, j, ca, cb), lo, True))
            else:
                kids += [(tr, q, j, ca, cm), (tr, q, j, cm, cb)]
        kv = ev(u, kids)
        windows += len(kids)
        best = min([rec["best"]] + [(hi, w[0], w[1], t) for w, (lo, hi, t) in zip(kids, kv) if hi < rng])
        nxt = [(w, lo, False) for w, (lo, hi, t) in zip(kids, kv) if lo < best[0]] + [x for x in terms if x[1] < best[0]]
        if len(nxt) > max_windows:
            truncated = True
            if trace is not None:
                trace.append((d + 1, None, None, len(nxt)))
            break
        d += 1
        live = nxt
        rec = dict(best=best, lo=min([best[0]] + [l for _, l, _ in live]), depth=d)
        if trace is not None:
            trace.append((d, rec["lo"], best[0], len(live)))
    hi, seg, q, t = rec["best"]
    found = q != math.inf
    return dict(lo=rec["lo"], hi=hi, time=t if found else -1.0, segment=seg if found else -1, depth=rec["depth"], windows=windows,
                live_empty=not live and not truncated, truncated=truncated, found=found)


def flags_of(r, offset, tol):
    return ((CONTACT if r["found"] and r["hi"] <= offset else 0) | (CLEAR if r["lo"] > offset else 0) |
            (CONVERGED if r["hi"] - r["lo"] <= tol or r["live_empty"] else 0) | (TRUNCATED if r["truncated"] else 0))


def pair_rows(pkg, pr, st, P, res, rng, offset, tol, max_depth=MAX_DEPTH, max_windows=None, owned=None, traces=None):
    """the rows in (robot, partner) order as a dict of numpy arrays [n].  rng, tol, max_depth, max_windows: the resolved values."""
    max_windows = pkg.PAIR_FRONTIER if max_windows is None else max_windows
    U = st["spline"].shape[0]
    ev = K._Eval(pkg, pr, st["spline"], st["piece_time"], P, res)
    rows = []
    for u in (range(U) if owned is None else owned):
        by = seeds_by_partner(ev, u, float(rng))
        for q in sorted(by):
            tr = [] if traces is not None else None
            r = search(ev, u, by[q][0], by[q][1], float(rng), float(tol), max_depth, max_windows, tr)
            if r is None:
                continue
            r.update(robot=u, partner=q)
            r["flags"] = flags_of(r, offset, tol)
            rows.append(r)
            if traces is not None:
                traces[(u, q)] = tr
    return {n: np.array([r[n] for r in rows], dtype=np.float64 if n in FIELDS[:3] else np.int32) for n in FIELDS}


def merge_symmetric(rows, rng, offset):
    """one row per unordered pair a < b with a listed direction: lo = min, hi = min over the two directions, a missing direction counting as `rng`
    (an unlisted direction is certified at least rng apart).  time, segment and `of` (whose flight the sample belongs to) from the direction with the
    smaller hi, on equality from (a, b).  depth = max, windows = sum; CONTACT / TRUNCATED of either, CLEAR / CONVERGED of both (a missing direction is
    converged, and clear iff rng > offset)."""
    by = {(int(rows["robot"][k]), int(rows["partner"][k])): {n: rows[n][k] for n in FIELDS} for k in range(len(rows["robot"]))}
    missing = dict(lo=rng, hi=rng, time=-1.0, segment=-1, depth=0, windows=0, flags=CONVERGED | (CLEAR if rng > offset else 0))
    out = []
    for a, b in sorted({(min(k), max(k)) for k in by}):
        x, y = by.get((a, b)), by.get((b, a))
        src, of = (x, a) if y is None or (x is not None and x["hi"] <= y["hi"]) else (y, b)
        x, y = x or missing, y or missing
        out.append(dict(robot=a, partner=b, lo=min(x["lo"], y["lo"]), hi=min(x["hi"], y["hi"]), time=src["time"], segment=src["segment"], of=of,
                        depth=max(x["depth"], y["depth"]), windows=x["windows"] + y["windows"],
                        flags=((x["flags"] | y["flags"]) & (CONTACT | TRUNCATED)) | (x["flags"] & y["flags"] & (CLEAR | CONVERGED))))
    names = ("lo", "hi", "time", "robot", "partner", "segment", "of", "depth", "flags", "windows")
    return {n: np.array([r[n] for r in out], dtype=np.float64 if n in names[:3] else np.int32) for n in names}


def default_tolerance(pkg, pr, names=("e2e_scn_b", "e2e_scn_c3", "e2e_scn_b_coupled"), rng=0.1 + 2 * 0.1, offset=0.1):
    """(widths per depth 0..40, floor depth, tolerance, largest live set of any pair at any depth, frontier, listed directed pairs per state): tol = 0,
    max_depth = 40 and no cap on the live set (MAX_WINDOWS) on the named end states; per depth the largest hi - lo over the listed pairs (a pair whose
    search has ended keeps its last bracket).  The floor and the tolerance by closest_ref.default_tolerance's rule; the frontier is the next power of two
    >= 4 x the largest live set, and at least 64."""
    widths, widest, listed = [0.0] * (MAX_DEPTH + 1), 0, {}
    for name in names:
        st, P, res = T.e2e_state(name)
        traces = {}
        rows = pair_rows(pkg, pr, st, P, res, rng, offset, 0.0, MAX_DEPTH, MAX_WINDOWS, traces=traces)
        listed[name] = len(rows["robot"])
        for tr in traces.values():
            widest = max(widest, max(t[3] for t in tr))
            for d in range(MAX_DEPTH + 1):
                _, lo, hi, _ = tr[min(d, len(tr) - 1)]
                widths[d] = max(widths[d], hi - lo)
    floor = next((d for d in range(MAX_DEPTH) if widths[d + 1] == 0.0 or not widths[d + 1] <= widths[d] / 2), MAX_DEPTH)
    frontier = max(64, 1 << max(0, math.ceil(math.log2(4 * max(widest, 1)))))
    return widths, floor, 10.0 ** math.ceil(math.log10(10 * widths[floor])), widest, frontier, listed


def orbit_state(pkg, scenes, radius=3.0, centre=(1.0, 2.0, 0.5), P=4):
    """a pair with a WIDE live set: robot 0 stays at `centre` for its whole flight, robot 1 flies a quarter circle of `radius` around it at constant angular
    speed (the spline space's least-squares fit of the arc: its radial error is asserted below 1e-6), both with piece_time 1.  The separation is the radius at
    every time, to that error, so no window of the pair can be dropped against another until its hull's sagitta (radius * angle^2 / 8, a quarter per round)
    falls below that error: the live set doubles per round for the first rounds.  (Two robots on the SAME net would not do: their separation is exactly 0 at the
    first sample, best.hi = 0, and no lo is below it -- the live set is empty at depth 0.)  Returns (scene, state)."""
    scene = dict(scenes.hard(U=2, n_points=500, pieces=P))
    st = R.port_state(scene, 0)
    conv = pkg.host_tables(P, 8)[0]
    s = np.linspace(0.0, 1.0, 41)
    bern = np.stack([math.comb(5, k) * s ** k * (1 - s) ** (5 - k) for k in range(6)], axis=1)      # [41][6]
    A = np.zeros((P * len(s), 3 * P + 3))
    for i in range(P):
        A[i * len(s):(i + 1) * len(s), 3 * i:3 * i + 6] = bern @ conv[i]
    ang = (0.5 * math.pi / P) * (np.arange(P)[:, None] + s[None, :]).ravel()
    c = np.asarray(centre, dtype=np.float64)
    target = c[None, :] + radius * np.stack([np.cos(ang), np.sin(ang), np.zeros_like(ang)], axis=1)
    net = np.linalg.lstsq(A, target, rcond=None)[0]                                                  # [T][3]
    assert np.abs(np.sqrt((((A @ net) - c) ** 2).sum(axis=1)) - radius).max() < 1e-6
    st["spline"][1] = net.T
    st["spline"][0] = np.linalg.lstsq(A, np.repeat(c[None, :], len(ang), axis=0), rcond=None)[0].T
    st["piece_time"][:] = 1.0
    assert R.valid_state(st, 2)
    return scene, st
