"""CPU: the numpy restatement of the BVH build and walk (tests/bvh_ref.py) checked against itself and against brute force, and the inputs of
tests/test_gpu_bvh_walk.py checked for substance -- so that a change of numpy's generators fails here, without a GPU, and not by a GPU test passing on nothing."""
import functools

import numpy as np
import pytest

import bvh_ref as B


@functools.lru_cache(maxsize=None)
def stats(name):
    """per (box, margin) of a case: candidates, hit boxes on the top level, largest frontier below it"""
    b = B.built(name)
    _, boxes, margins = B.case(name)
    ncand = np.array([[len(x) for x in per_margin] for per_margin in B.answers(name)]).T
    fr = np.array([[B.frontiers(b.levels, q, m) for m in margins] for q in boxes])          # [box][margin][level]
    return ncand, fr[:, :, -1], (fr[:, :, :-1].max(axis=2) if fr.shape[2] > 1 else np.zeros_like(ncand))


def test_level_rule_gives_one_to_five_levels_and_the_tile_edges():
    got = {n: B.level_counts(n) for n in B.POINT_SIZES}
    assert sorted({len(v) for v in got.values()}) == [1, 2, 3, 4, 5]
    assert got[512] == [64] and got[513] == [65, 9] and got[4096] == [512, 64] and got[4097] == [513, 65, 9]
    assert got[20000] == [2500, 313, 40] and got[32768] == [4096, 512, 64] and got[32769] == [4097, 513, 65, 9]
    assert got[262144] == [32768, 4096, 512, 64] and got[262145] == [32769, 4097, 513, 65, 9]
    assert {2047, 2048, 2049, 4096, 4097} <= set(B.POINT_SIZES)                               # one radix-sort tile is 2 048 keys


def test_outward_rounding_is_outward_and_tight():
    x = np.array([0.1, -0.1, 1000000.1, -70001.7, 1e-40, -1e-40, 0.0, 0.375, 1e-300, -1e-300])
    d, u = B.f32_down(x), B.f32_up(x)
    assert d.dtype == np.float32 and u.dtype == np.float32
    assert (d.astype(np.float64) <= x).all() and (u.astype(np.float64) >= x).all()
    exact = x.astype(np.float32).astype(np.float64) == x
    assert np.array_equal(d[exact], u[exact]) and np.array_equal(np.nextafter(d[~exact], np.float32(np.inf)), u[~exact])


@pytest.mark.parametrize("name", B.CASES)
def test_order_is_the_stable_sort_of_the_keys(name):
    b = B.built(name)
    assert np.array_equal(np.sort(b.order), np.arange(b.n))
    k = b.key[b.order]
    assert (k[1:] >= k[:-1]).all()
    tie = k[1:] == k[:-1]
    assert (b.order[1:][tie] > b.order[:-1][tie]).all()                                       # equal keys stay in index order
    if name == "copies":
        run = b.order[np.flatnonzero(b.order == B.DUP_SRC)[0]:][:B.DUP_N + 1]
        assert np.array_equal(run, np.r_[B.DUP_SRC, np.arange(B.DUP_AT, B.DUP_AT + B.DUP_N)])


@pytest.mark.parametrize("name", B.CASES)
def test_boxes_contain_what_is_under_them(name):
    b = B.built(name)
    assert [len(lo) for lo, _ in b.levels] == B.level_counts(b.n)
    llo, lhi = (x.astype(np.float64) for x in b.leaf)
    assert (llo <= b.plo).all() and (lhi >= b.phi).all()
    clo, chi, exact = llo, lhi, (b.plo, b.phi)
    for lo32, hi32 in b.levels:
        lo, hi = lo32.astype(np.float64), hi32.astype(np.float64)
        par = np.arange(len(clo)) // 8
        assert (lo[par] <= clo).all() and (hi[par] >= chi).all()                              # every parent box contains its children's boxes
        at = np.arange(0, len(exact[0]), 8)
        exact = (np.minimum.reduceat(exact[0], at, axis=0), np.maximum.reduceat(exact[1], at, axis=0))
        assert (lo <= exact[0]).all() and (hi >= exact[1]).all()                              # ... and every primitive under it
        assert (np.nextafter(lo32, np.float32(np.inf)).astype(np.float64) > exact[0]).all()   # rounded outward ONCE: by less than one float32 step
        assert (np.nextafter(hi32, np.float32(-np.inf)).astype(np.float64) < exact[1]).all()
        clo, chi = lo, hi


@pytest.mark.parametrize("name", B.CASES)
def test_walk_over_the_restated_pyramid_is_brute_force(name):
    b = B.built(name)
    verts, boxes, margins = B.case(name)
    for mi, m in enumerate(margins):
        for qi in range(len(boxes)):
            got, sizes = B.walk(b, boxes[qi], m)
            assert np.array_equal(got, B.answers(name)[mi][qi]), (m, qi)
            assert sizes[::-1] == B.frontiers(b.levels, boxes[qi], m), (m, qi)                 # a hit box has a hit parent: the frontier IS the level's hit boxes
    q = boxes[len(boxes) // 2]
    assert np.array_equal(B.candidates(verts, b.order, q, margins[-1]), B.answers(name)[-1][len(boxes) // 2])


def test_degenerate_triangles_have_the_point_clouds_answers():
    assert np.array_equal(B.built("tri4097_degenerate").order, B.built("pt4097").order)
    for a, b in zip(B.answers("tri4097_degenerate"), B.answers("pt4097")):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", B.CASES)
def test_inputs_are_not_vacuous(name):
    ncand, top, below = stats(name)
    b = B.built(name)
    assert (ncand > 0).mean() >= 0.45, (ncand > 0).mean()
    assert ncand.max() <= B.CAND_CAP and below.max() <= B.FRONT_CAP, (ncand.max(), below.max())
    if name in ("pt20000", "pt32768", "pt262144"):
        assert ((top > 8) & (ncand > 0)).sum() >= 20 and ((top <= 8) & (ncand > 0)).sum() >= 300, (((top > 8) & (ncand > 0)).sum(), ((top <= 8) & (ncand > 0)).sum())
    if len(b.levels) >= 3 and len(b.levels[-1][0]) == 9:
        assert (top[ncand > 0] <= 8).all()                                                    # every non-empty pair takes the double step
    if name == "copies":
        ids = np.arange(B.DUP_AT, B.DUP_AT + B.DUP_N)
        for per_margin in B.answers(name):
            for seq in per_margin[:20]:
                assert np.array_equal(seq[np.isin(seq, ids)], ids)                            # all 1 000, in index order: many rounds of the nc >= 64 flush
    if name == "tiny":
        _, boxes, _ = B.case(name)
        faces = {float(v) for v in np.unique(boxes[:, [0, 3]])}
        assert faces == {-1.0, -1e-40, 0.0, 1e-40, 1.0}
        lone = (boxes[:, 0] == boxes[:, 3]) & (ncand[:, 0] > 0)
        assert lone.sum() >= 5                                                                # zero-width boxes on a face that still find their points


def test_touching_boxes_touch():
    """the extra boxes of the far-away cases: at margin 0 their primitive passes by equality on all three axes"""
    for name in ("shift", "tri_shift"):
        verts, boxes, _ = B.case(name)
        v = verts[:, None, :] if verts.ndim == 2 else verts
        t = boxes[-40:]
        for q in t[:20]:
            assert (v.max(axis=1) == q[:3]).all(axis=1).any()
        for q in t[20:]:
            assert (v.min(axis=1) == q[3:]).all(axis=1).any()
        assert all(len(x) > 0 for x in B.answers(name)[0][-40:])


def test_capacity_edge_is_found():
    b = B.built("pt20000")
    h0, f0, h1, f1 = B.capacity_edge(b, 0.2)
    assert f0 <= B.FRONT_CAP < f1 and h0 < h1 and np.nextafter(h0, 2.0) == h1
    n0 = len(B.candidate_lists(b, [[-h0] * 3 + [h0] * 3], 0.2)[0])
    assert 0 < n0 <= 8192
