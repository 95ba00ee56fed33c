"""CPU: the shared assertions of tests/query_kit.py can fail.  Each is driven with small fakes -- a solver whose iterations are plain arithmetic, a group
whose answers are arrays, a command line whose output is canned, a library that counts its calls -- once where it must pass and once per way it must raise."""
import hashlib
import json
import types

import numpy as np
import pytest

import query_kit as K
from query_kit import STATE


def fake_pkg(log):
    """a package whose Solver iterates x -> 1.25 x + 0.1 on six arrays and counts 7 launches per iteration; `late` is hidden state that only the
    iterations from the seventh on read.  Every call is written to `log`; a second live solver is an error"""
    class Solver:
        live = 0

        def __init__(self, scene, stop=None):
            assert Solver.live == 0 and stop == 0.0
            Solver.live += 1
            self.x = {n: np.array([1.0, 2.0]) + i for i, n in enumerate(STATE)}
            self.iters = self.launches = self.bits = 0
            self.late = 0.0
            log.append("create")

        def _step(self, n):
            for _ in range(n):
                for v in self.x.values():
                    v *= 1.25
                    v += 0.1 + (self.late if self.iters >= 6 else 0.0)
                self.iters += 1
                self.launches += 7

        def iterate(self, n):
            log.append(("iterate", n))
            self._step(n)

        def iterate_async(self, n):
            log.append(("iterate_async", n))
            self._step(n)

        def sync(self):
            log.append("sync")

        def get_state(self):
            return {n: v.copy() for n, v in self.x.items()}

        def stats(self):
            return dict(iters=self.iters, error_bits=self.bits)

        def launch_count(self):
            return self.launches

        def close(self):
            Solver.live -= 1
            log.append("close")

    return types.SimpleNamespace(Solver=Solver)


def read_only(ask, then=3, log=None):
    log = [] if log is None else log

    def asked(how):
        def f(s):
            log.append(how)
            ask(s)
        return f

    K.assert_read_only(fake_pkg(log), "scene", asked("ask_async"), asked("ask_sync"), then=then)


def one_ulp(s):
    s.x["t_lambda"][1] = np.nextafter(s.x["t_lambda"][1], np.inf)


def set_bit(s):
    s.bits |= 4


def one_launch(s):
    s.launches += 1


def hidden(s):
    s.late = 1.0


def test_read_only_passes_and_calls_in_order():
    log = []
    read_only(lambda s: None, log=log)
    asking = ["create", ("iterate", 2), "ask_sync", ("iterate_async", 2), "ask_async", ("iterate", 2), "ask_sync", ("iterate", 3), "close"]
    silent = ["create", ("iterate", 2), ("iterate_async", 2), "sync", ("iterate", 2), ("iterate", 3), "close"]
    assert log == asking + silent          # the ask or sync() right behind the async batch; the first context closed before the second exists
    log = []
    read_only(lambda s: None, then=0, log=log)
    assert ("iterate", 3) not in log and log.count("close") == 2


@pytest.mark.parametrize("ask", [one_ulp, set_bit, one_launch, hidden])
def test_read_only_raises(ask):
    with pytest.raises(AssertionError):
        read_only(ask)


def test_read_only_continuation_is_what_finds_hidden_state():
    read_only(hidden, then=0)              # state, stats and launch count are equal: only the iterations after them differ
    with pytest.raises(AssertionError, match="more iterations"):
        read_only(hidden, then=3)
    with pytest.raises(AssertionError):
        read_only(one_ulp, then=0)


class Answers:
    """one context or a group: answers that depend on the iterations run and on the case; `tweak(a, its, case)` edits them"""

    def __init__(self, tweak=None):
        self.its, self.tweak = 0, tweak

    def iterate(self, n):
        self.its += n

    def ask(self, case):
        a = dict(lo=np.arange(4.0) + self.its + case, n_pairs=3 + self.its)
        if self.tweak:
            self.tweak(a, self.its, case)
        return a


def group_equals(tweak):
    return K.assert_group_equals(Answers(), Answers(tweak), lambda s, case: s.ask(case), ((0.0,), (0.5,)))


def test_group_equals():
    x = group_equals(None)
    assert x["n_pairs"] == 6 and np.array_equal(x["lo"], np.arange(4.0) + 3.5)      # one context's last answer: 3 iterations, the second case

    def element(a, its, case):
        a["lo"][2] = np.nextafter(a["lo"][2], 0.0)

    def extra_key(a, its, case):          # one context's answer lacks a key of the group's: no loop over its own keys sees that
        a["hi"] = a["lo"]

    def scalar(a, its, case):
        a["n_pairs"] += 1

    def late(a, its, case):
        if its == 3 and case == 0.5:
            a["lo"][0] += 1.0

    for tweak in (element, extra_key, scalar, late):
        with pytest.raises(AssertionError):
            group_equals(tweak)
    one, grp = Answers(), Answers(late)
    K.assert_group_equals(one, grp, lambda s, case: s.ask(case), ((0.0,), (0.5,)), its=(0,))
    assert one.its == grp.its == 0


PLAIN = ["iter 6", "ccd len: 1", "result written", ""]


class CannedCli(K.CliCase):
    """CliCase with the subprocess and the solver taken out: run() returns the canned lines, load() counts"""

    def __init__(self, flagged, group=None):
        self.flagged, self.group = flagged, flagged if group is None else group
        self.asked, self.loads, self._plain = [], 0, None

    def run(self, extra):
        self.asked.append(extra)
        if not extra:
            return list(PLAIN)
        return list(self.group if "--devices" in extra else self.flagged)

    def load(self):
        self.loads += 1


def test_queried_accepts_prefix_and_devices_lines():
    flagged = PLAIN[:2] + ["q uav 0 lo 1", "q fleet 1"] + PLAIN[2:]
    cli = CannedCli(flagged, ["devices: 0,0"] + flagged)
    got = list(cli.queried(["--q", "1e-6"], "q "))
    assert [e for e, _ in got] == [[], ["--devices", "0,0"]] and got[0][1] == flagged and cli.loads == 2
    assert cli.asked == [["--q", "1e-6"], [], ["--q", "1e-6", "--devices", "0,0"]]      # the plain run once
    other = PLAIN[:1] + ["p 0"] + PLAIN[1:]
    cli = CannedCli(PLAIN[:1] + ["p 0", "q uav 0"] + PLAIN[1:])
    assert len(list(cli.queried(["--p", "--q"], "q ", against=other))) == 2 and [] not in cli.asked


@pytest.mark.parametrize("how", ["extra", "changed", "missing", "group_only"])
def test_queried_raises_on_a_foreign_line(how):
    good = PLAIN[:2] + ["q uav 0 lo 1"] + PLAIN[2:]
    bad = {"extra": good[:1] + ["warning: x"] + good[1:], "changed": ["iter 7"] + good[1:], "missing": good[:1] + good[2:], "group_only": good}[how]
    cli = CannedCli(bad, good[:3] + ["queue 2"] + good[3:] if how == "group_only" else None)
    with pytest.raises(AssertionError):
        list(cli.queried(["--q"], "q "))
    assert cli.loads == (1 if how == "group_only" else 0)


def test_load_dump_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    U, P = 3, 2
    T = 3 * P + 3
    st = {n: rng.normal(size=s) for n, s in zip(STATE, ((U, 3, T), (U, 3, 6 * P), (U, 3, 6 * P), (U, P), (U, P), (U,)))}
    want = {n: v.copy() for n, v in st.items()}
    want["spline"], want["piece_time"] = rng.normal(size=(U, 3, T)) * 1e3 / 3.0, rng.uniform(0.1, 30.0, U)
    with open(tmp_path / "state.txt", "w") as f:
        f.write("uav_num %d piece_num %d iter 6 gnorm 0.5 converged 0\n" % (U, P))
        for u in range(U):
            f.write("uav %d piece_time %.17g\n" % (u, want["piece_time"][u]))
            for r in range(T):
                f.write("%.17g %.17g %.17g\n" % tuple(want["spline"][u][:, r]))
    got = K.load_dump(tmp_path / "state.txt", st)
    assert set(got) == set(STATE) and all(np.array_equal(got[n], want[n]) for n in STATE)
    assert not np.array_equal(st["spline"], want["spline"])          # the state handed in is left as it was


def test_reference_config():
    text = K.reference_config()
    assert len(text) == 192 and hashlib.sha256(text.encode()).hexdigest() == "4f976d454582cb1a8cae16214f0684180e1255093fe1f19ba798558e838257f8"
    base = json.loads(text)
    assert list(base) == ["auto", "init", "gui", "optimal_plane", "decouple", "res", "vel_limit", "acc_limit", "lambda", "epsilon", "margin", "offset", "stop",
                          "exit", "init_ob", "mu"]
    assert base == dict(auto=0, init=1, gui=0, optimal_plane=0, decouple=1, res=8, vel_limit=2, acc_limit=2, epsilon=0.1, margin=0.1, offset=0.1, stop=0.01,
                        exit=0, init_ob=1, mu=0.1, **{"lambda": 10.0})
    assert K.reference_config(init=2) == text.replace('"init":1', '"init":2') != text and json.loads(K.reference_config(init=2)) == dict(base, init=2)
    assert json.loads(K.reference_config(optimal_plane=1, decouple=0)) == dict(base, optimal_plane=1, decouple=0)
    with pytest.raises(AssertionError):
        K.reference_config(no_such_key=1)


def test_close_to_six_digits():
    assert K.close_to_six_digits("1.234567", 1.2345678) and not K.close_to_six_digits("1.23457", 1.2345678)      # 1e-6 of the value, no more
    assert K.close_to_six_digits("-2.5e-07", -2.5000001e-07) and not K.close_to_six_digits("1e-13", 0.0) and K.close_to_six_digits("1e-13", 0.0, floor=1e-12)


class CountingLib:
    def __init__(self):
        self.calls = []

    def tj_default_params(self, tp, mode, uav_num, piece_num):
        self.calls.append(("default_params", mode, uav_num, piece_num))

    def tj_create(self, tp, ctx):
        self.calls.append("create")
        return 0

    def tj_init_state(self, ctx, wp, piece_time):
        self.calls.append(("init_state", piece_time.value))
        return 0

    def tj_destroy(self, ctx):
        self.calls.append("destroy")


def test_raw_context_destroys_its_context_when_the_body_raises():
    import ctypes as C
    lib = CountingLib()
    pkg = types.SimpleNamespace(load_library=lambda: lib, TjParams=C.c_int)
    scenes = types.SimpleNamespace(tiny=lambda mode: dict(waypoints=np.zeros((3, 2, 3))))
    with pytest.raises(ZeroDivisionError):
        with K.raw_context(pkg, scenes) as (got, ctx, init):
            assert got is lib and lib.calls == [("default_params", 1, 3, 5), "create"]
            init()
            1 / 0
    assert lib.calls == [("default_params", 1, 3, 5), "create", ("init_state", 20.0), "destroy"]
    with K.raw_context(pkg, scenes):
        pass
    assert lib.calls[-2:] == ["create", "destroy"]
