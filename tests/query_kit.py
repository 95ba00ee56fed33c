"""What the tests of the read-only queries (tests/test_gpu_<query>.py) share, stated once: the read-only proof, the group comparison, the raw-context
preamble of test_bad_arguments and the command-line case.  Plain functions with explicit arguments, imported by bare name like the *_ref modules; what is
specific to one query (its restatement, its states, its fields) stays in that query's file.  tests/test_query_kit.py drives every assertion here with
fakes, on the CPU, to show that it can fail."""
import contextlib
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

STATE = ("spline", "p_slack", "p_lambda", "t_slack", "t_lambda", "piece_time")
MESH = "x.obj"


def pkg_module():
    return importlib.import_module("traj-opt-admm_amd")


def loaded(pkg, scene, st, params=None):
    """a Solver(stop=0.0) that holds `st`; arrays `st` does not name (a constructed state may give spline and piece_time only) stay the solver's own"""
    slv = pkg.Solver(scene, params, stop=0.0) if params else pkg.Solver(scene, stop=0.0)
    slv.set_state({**slv.get_state(), **st})
    return slv


def one_queue(monkeypatch):
    """the one-queue chain: neither the x-solve nor k_front on a queue of its own"""
    monkeypatch.setenv("TJ_XS_ASYNC", "0")
    monkeypatch.setenv("TJ_FRONT_ASYNC", "0")


def assert_read_only(pkg, scene, ask_async, ask_sync, then=3):
    """2 + 2 + 2 iterations twice, once asking and once not: ask_sync(s) behind each iterate(2), ask_async(s) right behind iterate_async(2) (the query drains
    the queues itself; the other run calls sync()).  The six state arrays, stats() and launch_count() are equal, and so is the state `then` iterations on"""

    def run(asked):   # one context at a time: a second live context may find the process's hardware-queue budget taken and keep the one-queue chain (tj_create)
        s = pkg.Solver(scene, stop=0.0)
        for k in range(3):
            if k == 1:
                s.iterate_async(2)
                if asked:
                    ask_async(s)
                else:
                    s.sync()
            else:
                s.iterate(2)
                if asked:
                    ask_sync(s)
        out = s.get_state(), s.stats(), s.launch_count()
        if then:
            s.iterate(then)
        out += (s.get_state(),)
        s.close()
        return out

    (sa, ta, la, na), (sb, tb, lb, nb) = run(True), run(False)
    for n in STATE:
        assert np.array_equal(sa[n], sb[n]), n
        assert np.array_equal(na[n], nb[n]), (n, "after %d more iterations" % then)
    assert ta == tb
    assert la == lb


@contextlib.contextmanager
def raw_context(pkg, scenes):
    """(lib, ctx, init): a context of 3 robots, 5 pieces through the C ABI, no state yet; init() is tj_init_state with tiny(mode=1)'s waypoints and 20.0.
    tj_destroy on the way out, whatever the block raised"""
    lib = pkg.load_library()
    tp = pkg.TjParams()
    lib.tj_default_params(C.byref(tp), 1, 3, 5)
    ctx = C.c_void_p()
    assert lib.tj_create(C.byref(tp), C.byref(ctx)) == 0

    def init():
        wp = np.ascontiguousarray(scenes.tiny(mode=1)["waypoints"])
        assert lib.tj_init_state(ctx, wp.ctypes.data_as(C.POINTER(C.c_double)), C.c_double(20.0)) == 0

    try:
        yield lib, ctx, init
    finally:
        lib.tj_destroy(ctx)


def assert_sharded_refuses(pkg, scenes, call, group_name):
    """a plain sharded context does not hold the other ranks' piece_time: TJ_ERR_UNSUPPORTED (-5), and the message names the group call"""
    half = pkg.Solver(scenes.hard(), stop=0.0, rank=1, world=2)
    try:
        with pytest.raises(pkg.TrajAdmmError) as ei:
            call(half)
        assert "-5" in str(ei.value) and group_name in str(ei.value)
    finally:
        half.close()


def group_pair(pkg, scene, ranks):
    """one context and a group of `ranks` ranks on device 0, both at the initial state"""
    return pkg.Solver(scene, stop=0.0), pkg.Group(scene, [0] * ranks, stop=0.0)


def assert_group_equals(one, grp, ask, cases, its=(0, 3)):
    """ask(s, *case) of the group == of one context for every case, the same keys and every field bit for bit, after each of `its` further iterations;
    returns one context's last answer"""
    for it in its:
        if it:
            one.iterate(it)
            grp.iterate(it)
        for case in cases:
            x, y = ask(one, *case), ask(grp, *case)
            assert set(x) == set(y), (it, case)
            for k in x:
                assert np.array_equal(x[k], y[k]), (it, case, k)
    return x


_CONFIG = ('{"auto":0,"init":1,"gui":0,"optimal_plane":0,"decouple":1,"res":8,"vel_limit":2,"acc_limit":2,"lambda":1e1,'
           '"epsilon":1e-1,"margin":1e-1,"offset":1e-1,"stop":1e-2,"exit":0,"init_ob":1,"mu":0.1}')


def reference_config(**overrides):
    """the text of Config_File/3D.json: the shipped values with gui off, all 16 keys; an override replaces one key's value"""
    text = _CONFIG
    for key, value in overrides.items():
        text, n = re.subn('"%s":[^,}]+' % key, '"%s":%s' % (key, value), text)
        assert n == 1, key
    return text


def load_dump(path, st):
    """--dump-state file -> the solver state `st` with its control points and piece_time replaced (17 digits: the exact doubles)"""
    lines = open(path).read().strip().split("\n")
    U, P = int(lines[0].split()[1]), int(lines[0].split()[3])
    T = 3 * P + 3
    out = {k: v.copy() for k, v in st.items()}
    for u in range(U):
        blk = lines[1 + u * (T + 1):1 + (u + 1) * (T + 1)]
        assert blk[0].split()[:2] == ["uav", str(u)]
        out["piece_time"][u] = float(blk[0].split()[3])
        out["spline"][u] = np.array([[float(x) for x in l.split()] for l in blk[1:]]).T
    return out


def close_to_six_digits(word, value, floor=0.0):
    """a double the command line printed with 6 significant digits against the library's"""
    return abs(float(word) - value) <= 1e-6 * abs(value) + floor


def assert_only_adds(lines, prefix, plain):
    """a flag adds its own lines (and a group its `devices:` line) and changes no other"""
    assert [l for l in lines if not l.startswith(prefix) and not l.startswith("devices:")] == plain


class CliCase:
    """One of the mains in a directory with the scene's files (tiny(mode=1) unless given) and Config_File/3D.json, and one Solver on the same scene to ask
    about the state a run dumped"""

    def __init__(self, pkg, scenes, tmp_path, scene=None, exe="multiPathPlanning3D", **config):
        self.scene = scenes.tiny(mode=1) if scene is None else scene
        self.cwd = tmp_path
        scenes.write_reference_files(self.scene, str(tmp_path), MESH)
        os.makedirs(tmp_path / "Config_File", exist_ok=True)
        (tmp_path / "Config_File" / "3D.json").write_text(reference_config(**config))
        self.exe = os.path.join(ROOT, "traj-opt-admm_amd", exe)
        self.slv = pkg.Solver(self.scene, stop=0.0)
        self._plain = None

    def run(self, extra):
        """6 iterations with the state dumped: the output's lines but the wall-clock ones (2: not converged, everything is printed all the same)"""
        r = subprocess.run([self.exe, MESH, "--max-iter", "6", "--dump-state", "state.txt"] + extra, cwd=self.cwd, capture_output=True, text=True, timeout=300)
        assert r.returncode in (0, 2), r.stderr
        return [l for l in r.stdout.split("\n") if not l.startswith("time:")]

    @property
    def plain(self):
        """the run without a flag, started once, when first asked for"""
        if self._plain is None:
            self._plain = self.run([])
        return self._plain

    def load(self):
        """the solver takes the state the last run dumped"""
        self.slv.set_state(load_dump(self.cwd / "state.txt", self.slv.get_state()))

    def queried(self, flag_args, prefix, against=None):
        """runs with `flag_args` on one context and on a two-rank group: every line that starts with neither `prefix` nor `devices:` is a line of the run
        without a flag (or of `against`, the lines of another run); yields (extra, lines) with the dumped state loaded into the solver"""
        for extra in ([], ["--devices", "0,0"]):
            lines = self.run(flag_args + extra)
            assert_only_adds(lines, prefix, self.plain if against is None else against)
            self.load()
            yield extra, lines

    def close(self):
        self.slv.close()
