"""Known answers for the obstacle BVH (csrc/kernels_bvh.h, host_tables.h build_bvh) and its walk (csrc/kernels_sep.h bvh_query), restated in numpy
(plain module: no fixtures, no tests, no GPU, nothing of the reference project).

  build        the Morton sort and the box pyramid, expression by expression: centroid, per-axis extent, 21-bit quantisation, bit interleave, STABLE sort
               (= the lexicographic (key, index) order of both builds), the level rule of set_obstacles, fp64 unions rounded outward to float32 once.
  candidates   what a query returns with sort=False: the walk ends in the fp64 leaf test `x + m < q.lo[k]` / `x > q.hi[k] + m` on the primitive itself (a
               point, or the fp64 min / max of a triangle's three vertices), frontiers are compacted in ascending order and leaves are taken slot by slot,
               then by lane -- so the sequence is the passing positions of the sorted order, ascending, mapped through `order`.  No tolerance anywhere.
  frontiers    hit boxes per level by box_near's expression on the float32 boxes widened to double: what the walk's frontier holds (FRONT_CAP).
  walk         the level-by-level walk over the restated pyramid (tests/test_bvh_ref.py: it must give the brute-force set).
  cloud, queries, touching, case
               the inputs of tests/test_gpu_bvh_walk.py; tests/test_bvh_ref.py checks on the CPU that they do not let a test pass on nothing.
What none of this covers: the `visits` counter of the walk (a statistic: it depends on the form of the walk, not on the candidate set)."""
import functools
from types import SimpleNamespace

import numpy as np

MARGINS = (0.0, 0.1, 0.2)
POINT_SIZES = (1, 7, 8, 9, 64, 65, 512, 513, 2047, 2048, 2049, 4096, 4097, 20000, 32768, 32769, 262144, 262145)
TRI_SIZES = (1, 9, 513, 4097, 32769)
SHIFT = (4097.3, -70001.7, 1000000.1)
FRONT_CAP = 1024      # dev_common.h
CAND_CAP = 2048       # Solver.kat_query's default `cap`
U64 = np.uint64


def spread21(v):
    """dev_spread21"""
    v = v.astype(U64) & U64(0x1fffff)
    v = (v | v << U64(32)) & U64(0x1f00000000ffff)
    v = (v | v << U64(16)) & U64(0x1f0000ff0000ff)
    v = (v | v << U64(8)) & U64(0x100f00f00f00f00f)
    v = (v | v << U64(4)) & U64(0x10c30c30c30c30c3)
    v = (v | v << U64(2)) & U64(0x1249249249249249)
    return v


def f32_down(x):
    """largest float32 <= x"""
    f = x.astype(np.float32)
    return np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f)


def f32_up(x):
    """smallest float32 >= x"""
    f = x.astype(np.float32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f)


def level_counts(n):
    """set_obstacles: level 0 = boxes over 8 consecutive primitives, up to a top level of <= 64 boxes"""
    out, cnt = [], (n + 7) // 8
    while True:
        out.append(cnt)
        if cnt <= 64:
            return out
        cnt = (cnt + 7) // 8


def _prims(verts):
    v = np.ascontiguousarray(verts, dtype=np.float64)
    return v[:, None, :] if v.ndim == 2 else v


def morton_keys(verts):
    v = _prims(verts)
    cen = v[:, 0, :] if v.shape[1] == 1 else (v[:, 0, :] + v[:, 1, :] + v[:, 2, :]) / 3.0
    lo, hi = cen.min(axis=0), cen.max(axis=0)
    key = np.zeros(len(v), dtype=U64)
    for k in range(3):
        ext = hi[k] - lo[k]
        f = (cen[:, k] - lo[k]) / ext if ext > 0 else np.zeros(len(v))
        q = np.trunc(np.minimum(2097151.0, np.maximum(0.0, f * 2097152.0))).astype(U64)
        key |= spread21(q) << U64(k)
    return key


def build(verts):
    """verts [N][3] or [N][prim][3] -> order [N] (sorted position -> caller's index), key [N], plo / phi [N][3] (fp64 box of every primitive, sorted
    order), levels = [(lo32 [cnt][3], hi32 [cnt][3]) ...] from level 0 up, leaf = (lo32, hi32) [N][3] of the primitives"""
    v = _prims(verts)
    n = len(v)
    key = morton_keys(v)
    order = np.argsort(key, kind="stable")
    s = v[order]
    plo, phi = s.min(axis=1), s.max(axis=1)
    levels, lo, hi = [], plo, phi
    for cnt in level_counts(n):
        at = np.arange(0, len(lo), 8)
        lo, hi = np.minimum.reduceat(lo, at, axis=0), np.maximum.reduceat(hi, at, axis=0)     # unions in fp64 ...
        assert len(lo) == cnt
        levels.append((f32_down(lo), f32_up(hi)))                                              # ... rounded outward once per box
    return SimpleNamespace(n=n, prim=v.shape[1], order=order, key=key, plo=plo, phi=phi, levels=levels, leaf=(f32_down(plo), f32_up(phi)))


def _passing(lo, hi, q, m):
    """ascending positions whose box [lo, hi] passes `hi + m < q.lo[k]` / `lo > q.hi[k] + m` on no axis (lo, hi: [3][n], contiguous rows)"""
    idx = None
    for k in range(3):
        l, h = (lo[k], hi[k]) if idx is None else (lo[k][idx], hi[k][idx])
        ok = np.flatnonzero(~((h + m < q[k]) | (l > q[3 + k] + m)))
        idx = ok if idx is None else idx[ok]
    return idx


def candidates(verts, order, q, m):
    """q = (lo.xyz, hi.xyz): the device's candidate sequence with sort=False"""
    s = _prims(verts)[order]
    return order[_passing(np.ascontiguousarray(s.min(axis=1).T), np.ascontiguousarray(s.max(axis=1).T), np.asarray(q, dtype=np.float64), float(m))]


def candidate_lists(b, boxes, m):
    """candidates() of every row of boxes [nq][6] on a finished build"""
    lo, hi = np.ascontiguousarray(b.plo.T), np.ascontiguousarray(b.phi.T)
    return [b.order[_passing(lo, hi, q, float(m))] for q in np.asarray(boxes, dtype=np.float64).reshape(-1, 6)]


def frontiers(levels, q, m):
    """hit boxes per level (level 0 first) by box_near's expression"""
    q = np.asarray(q, dtype=np.float64)
    return [len(_passing(np.ascontiguousarray(lo.astype(np.float64).T), np.ascontiguousarray(hi.astype(np.float64).T), q, float(m))) for lo, hi in levels]


def walk(b, q, m):
    """the walk over the restated pyramid: hit boxes level by level from the top (children of hit boxes only), the float32 leaf boxes for triangles, then
    the fp64 leaf test.  Returns (candidate sequence, frontier sizes from the top level down to level 0)."""
    q = np.asarray(q, dtype=np.float64); m = float(m)

    def hit(lo, hi, idx):
        lo = lo[idx].astype(np.float64); hi = hi[idx].astype(np.float64)
        return idx[~((hi + m < q[:3]) | (lo > q[3:] + m)).any(axis=1)]
    top = len(b.levels) - 1
    front = hit(*b.levels[top], np.arange(len(b.levels[top][0])))
    sizes = [len(front)]
    for lv in range(top - 1, -1, -1):
        child = (front[:, None] * 8 + np.arange(8)).ravel()
        front = hit(*b.levels[lv], child[child < len(b.levels[lv][0])])
        sizes.append(len(front))
    pt = (front[:, None] * 8 + np.arange(8)).ravel()
    pt = pt[pt < b.n]
    if b.prim == 3:
        pt = hit(*b.leaf, pt)
    return b.order[hit(b.plo, b.phi, pt)], sizes


# ---- the inputs ----
def cloud(N, seed, shift=0):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-3, 3, (N, 3))
    p[:N // 4] = np.round(p[:N // 4] * 8) / 8       # a lattice quarter: with the lattice queries, faces touch points exactly
    p += shift
    return p


def queries(pts, N, seed, nq=200):
    rng = np.random.default_rng(seed + 1)
    sc = min(1, (20000 / N) ** (1 / 3))
    ext = rng.uniform(0, 1, (nq, 3)) * rng.choice([0.05, 0.3, 1.5], (nq, 1)) * sc
    lo = rng.uniform(pts.min(0) - 0.2, pts.max(0) + 0.2, (nq, 3))
    lo[:nq // 2] = pts[rng.integers(0, N, nq // 2)] - ext[:nq // 2] / 2
    lo[-50:] = np.round(lo[-50:] * 8) / 8
    ext[-50:] = np.round(ext[-50:] * 8) / 8
    return np.concatenate([lo, lo + ext], axis=1)


def touching(verts, seed, n=40):
    """boxes with a corner exactly on a primitive's own fp64 box: the first half has lo = the primitive's max (it grows upward), the second half has hi = the
    primitive's min.  At margin 0 the primitive passes the leaf test by equality, so it is lost as soon as a box above it is rounded inward on any axis."""
    v = _prims(verts)
    rng = np.random.default_rng(seed + 2)
    pick = rng.integers(0, len(v), n)
    ext = rng.uniform(0.05, 0.5, (n, 3))
    lo, hi = v[pick].max(axis=1), v[pick].min(axis=1)
    up = np.concatenate([lo, lo + ext], axis=1); down = np.concatenate([hi - ext, hi], axis=1)
    return np.where((np.arange(n) < n // 2)[:, None], up, down)


def triangles(N, seed, shift=0):
    return cloud(N, seed, shift)[:, None, :] + np.random.default_rng(5).normal(0, 0.05, (N, 3, 3))


DUP_AT, DUP_N, DUP_SRC = 1500, 1000, 17      # the `copies` case: cloud[1500:2500] = cloud[17]


def _seed(N):
    return 7000 + N


@functools.lru_cache(maxsize=None)
def case(name):
    """-> verts ([N][3] points or [N][3][3] triangles), boxes [nq][6], margins.  Names: pt<N>, tri<N>, tri4097_degenerate (three equal vertices: the
    answers of pt4097), and at N = 4097: shift / tri_shift (far from the origin), flat_z (all z equal), line (y and z constant), copies (1 000 copies
    of one point), tiny (coordinates of 0 and +-1e-40 on x, query faces at 0 and +-1e-40, margin 0)."""
    margins = MARGINS
    if name.startswith("pt") or name.startswith("tri") and name[3:].isdigit():
        N = int(name[2:] if name.startswith("pt") else name[3:])
        pts = cloud(N, _seed(N))
        verts = pts if name.startswith("pt") else triangles(N, _seed(N))
        boxes = queries(pts, N, _seed(N))
    else:
        N = 4097
        pts = cloud(N, _seed(N), SHIFT if "shift" in name else 0)
        if name == "flat_z":
            pts[:, 2] = 0.375
        elif name == "line":
            pts[:, 1] = -1.25; pts[:, 2] = 0.375
        elif name == "copies":
            pts[DUP_AT:DUP_AT + DUP_N] = pts[DUP_SRC]
        elif name == "tiny":
            pts[:, 0] = np.random.default_rng(3).choice([-1e-40, 0.0, 1e-40], N)
        boxes = queries(pts, N, _seed(N))
        verts = pts
        if name == "tri4097_degenerate":
            verts = np.repeat(pts[:, None, :], 3, axis=1)
        elif name == "tri_shift":
            verts = triangles(N, _seed(N), SHIFT)
        elif name == "copies":                       # twenty boxes around the copied point
            ext = boxes[:20, 3:] - boxes[:20, :3]
            boxes[:20, :3] = pts[DUP_SRC] - ext / 2; boxes[:20, 3:] = boxes[:20, :3] + ext
        elif name == "tiny":
            rng = np.random.default_rng(4)
            a = rng.choice([-1.0, -1e-40, 0.0, 1e-40, 1.0], (len(boxes), 2))
            boxes[:, 0] = a.min(axis=1); boxes[:, 3] = a.max(axis=1)
            margins = (0.0,)
        if "shift" in name:
            boxes = np.concatenate([boxes, touching(verts, _seed(N))])
    return np.ascontiguousarray(verts), np.ascontiguousarray(boxes), margins


POINT_CASES = tuple(f"pt{n}" for n in POINT_SIZES)
TRI_CASES = tuple(f"tri{n}" for n in TRI_SIZES) + ("tri4097_degenerate",)
EDGE_CASES = ("shift", "tri_shift", "flat_z", "line", "copies", "tiny")
CASES = POINT_CASES + TRI_CASES + EDGE_CASES


@functools.lru_cache(maxsize=None)
def built(name):
    return build(case(name)[0])


@functools.lru_cache(maxsize=None)
def answers(name):
    """per margin of the case: the candidate sequence of every box -- computed once and shared"""
    _, boxes, margins = case(name)
    return [candidate_lists(built(name), boxes, m) for m in margins]


def capacity_edge(b, m, lo=1.6, hi=1.8):
    """the cubes [-h, h]^3 on either side of FRONT_CAP, by bisection on h down to neighbouring doubles: (h_pass, frontier, h_fail, frontier) where frontier
    = the largest number of hit boxes on a level below the top one (those are the frontiers the walk compacts into its FRONT_CAP slots)"""
    def worst(h):
        return max(frontiers(b.levels[:-1], [-h, -h, -h, h, h, h], m))
    assert worst(lo) <= FRONT_CAP < worst(hi)
    while True:
        mid = 0.5 * (lo + hi)
        if not lo < mid < hi:
            return lo, worst(lo), hi, worst(hi)
        if worst(mid) <= FRONT_CAP:
            lo = mid
        else:
            hi = mid
