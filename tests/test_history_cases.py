"""CPU: the probe registry of the handle-history tests (tests/history_cases.py) held to its own laws.

  * BUFFERS has exactly the plda::DevBuf members of plda_handle (plda_amd/csrc/common.hpp read as text): a buffer added
    later without a history probe, or a reason, fails here;
  * a probe's inputs are a function of its name (and the model's dimensions) alone;
  * the detector can fail: the harness that tests/test_gpu_handle_history.py runs on the device is run here against small
    fake engines written in Python.  Every family accepts the honest fake and rejects at least one that breaks the law in
    the way the family looks for: one keeps the tail of a larger earlier input, one keeps a table keyed on a pointer but not
    on the model, one returns the previous result after a refused call."""
import os

import numpy as np
import pytest

import history_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- the registry
def test_buffers_are_the_handles():
    with open(os.path.join(ROOT, "plda_amd", "csrc", "common.hpp")) as f:
        members = H.handle_buffers(f.read())
    assert len(members) == len(set(members)) and len(members) > 90
    assert "hio_O" in members and "eer_list" in members
    assert sorted(H.BUFFERS) == sorted(members), (sorted(set(members) - set(H.BUFFERS)), sorted(set(H.BUFFERS) - set(members)))
    for buf, use in H.BUFFERS.items():
        if isinstance(use, str):
            assert len(use) > 20 and "\n" not in use, buf          # a one-line reason
        else:
            assert use and all(name in H.PROBES for name in use), buf
    # SHARED is derived: every buffer whose probes come from two modules or more gets neighbour pairs, or is exempt by name
    for buf, use in H.BUFFERS.items():
        shared = not isinstance(use, str) and len({H.PROBES[n].module for n in use}) >= 2
        assert (buf in H.SHARED) == (shared and buf not in H.NOT_NEIGHBOURS), buf
    assert all(len(why) > 20 for why in H.NOT_NEIGHBOURS.values())
    for buf in ("host_flag", "calib_part", "sn_slab", "trial_hist", "linalg_part", "bt4_cnt", "s_A16"):
        assert buf in H.SHARED, buf
    for buf, sw in H.UNDER.items():              # a buffer behind a switch: its probes run, and are compared, under it
        assert not isinstance(H.BUFFERS[buf], str) and sw in (H.BF16X3, H.BT4)
    assert all(isinstance(H.BUFFERS[b], str) for b in ("comm_mm", "comm_mc", "comm_counts", "comm_hist", "timeline"))


def test_families_have_a_large_and_a_small_probe():
    for family, f in H.FAMILIES.items():
        assert {"large", "small"} <= set(f) <= {"large", "small", "third"}, family
        assert len(set(f.values())) == len(f) and all(n in H.PROBES for n in f.values()), family
        mods = {H.PROBES[n].module for n in f.values()}
        assert len(mods) == 1, (family, mods)
    in_family = {n for f in H.FAMILIES.values() for n in f.values()}
    named = {n for use in H.BUFFERS.values() if not isinstance(use, str) for n in use}
    assert named <= set(H.PROBES)
    # every probe is reached by the shrink-and-regrow family, the neighbours or the model routes
    assert set(H.PROBES) - in_family <= {"transform.truncated", "transform.L300", "embed.centre", "fit.split"}


def test_small_probes_are_strictly_smaller():
    """every array a small probe builds is no larger than the large one's, and the inputs in total are smaller"""
    for family, f in H.FAMILIES.items():
        big, small = H.PROBES[f["large"]], H.PROBES[f["small"]]
        a = big.inputs(*(H.MODELS[big.home][:2] if big.home else (0, 0)))
        b = small.inputs(*(H.MODELS[small.home][:2] if small.home else (0, 0)))
        size = lambda d: sum(np.asarray(v).size for v in d.values())      # noqa: E731
        assert size(b) < size(a), family
        for k in set(a) & set(b):
            assert np.asarray(b[k]).size <= np.asarray(a[k]).size, (family, k)


@pytest.mark.parametrize("name", sorted(H.PROBES))
def test_probe_inputs_are_deterministic(name):
    p = H.PROBES[name]
    dims = H.MODELS[p.home][:2] if p.home else (0, 0)
    a, b = p.inputs(*dims, cached=False), p.inputs(*dims, cached=False)
    assert sorted(a) == sorted(b)
    for k in a:
        u, v = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (name, k)
    if p.home:                                   # another model dimension: other inputs
        other = p.inputs(dims[0] + 1, dims[1] + 1, cached=False)
        assert any(np.asarray(other[k]).tobytes() != np.asarray(a[k]).tobytes() for k in a)


def test_models_and_walks_are_functions_of_their_seed():
    for key, (din, dout, _) in H.MODELS.items():
        m1, m2 = H.model(key), H.model(key)
        assert m1[1].shape == (dout, din) and all(np.array_equal(u, v) for u, v in zip(m1, m2))
    args = (H.WALK_PROBES, sorted(H.ROUTES), sorted(H.REFUSALS))
    assert set(H.PROBES) - set(H.WALK_PROBES) == {"bt4.large", "bt4.small"}
    a, b = H.walk_steps(0, 48, *args), H.walk_steps(0, 48, *args)
    assert a == b and len(a) == 48 and a != H.walk_steps(1, 48, *args)
    assert [s[0] for s in a] == [i % 2 for i in range(48)]                  # the two handles alternate
    assert {s[1] for s in a} == {"probe", "route", "refuse", "stream"}
    for which in (0, 1):                         # each handle moves to a side stream AND back, and is probed after either
        mine = [s for s in a if s[0] == which]
        for where in ("side", "own"):
            at = [i for i, s in enumerate(mine) if s[1:] == ("stream", where)]
            assert at and any(s[1] == "probe" for s in mine[at[0]:]), (which, where)
    for _, kind, name in a:
        assert name in {"probe": H.PROBES, "route": H.ROUTES, "refuse": H.REFUSALS, "stream": ("side", "own")}[kind]
    for call, own, other, home in H.REFUSALS.values():
        assert own in H.PROBES and other in H.PROBES and H.PROBES[own].module != H.PROBES[other].module
        assert home is None or home in H.MODELS


# ------------------------------------------------------------------------------------------- the detector can fail
class FakeError(Exception):
    pass


class FakeEngine(object):
    """A handle in miniature: one growable scratch buffer shared by two `modules`, a coefficient table cached per input
    `pointer`, a model with an epoch.  flaw: None (honest), "tail", "pointer" or "refused"."""

    def __init__(self, flaw=None):
        self.flaw, self.scratch, self.used = flaw, np.zeros(0), 0
        self.mean = self.t = self.psi = None
        self.epoch, self.table, self.table_key = 0, None, None
        self.last, self.stale = None, False

    # the model
    def set_model(self, mean, t, psi):
        self.mean, self.t, self.psi = (np.array(a, np.float64) for a in (mean, t, psi))
        self.epoch += 1

    def dims(self):
        return self.t.shape

    def get_model(self):
        if self.mean is None:
            raise FakeError("not fitted")
        return dict(mean=self.mean, transform=self.t, psi=self.psi)

    # two modules over one scratch buffer
    def _stage(self, x):
        if len(x) > len(self.scratch):
            self.scratch = np.zeros(len(x))           # (an allocation is fresh memory)
            self.used = 0
        self.scratch[:len(x)] = x
        n = max(len(x), self.used) if self.flaw == "tail" else len(x)      # the flaw: the rows an earlier call left count too
        self.used = max(self.used, len(x))
        return self.scratch[:n]

    def total(self, x):
        return self._answer(np.array([self._stage(x).sum()]))

    def peak(self, x):
        return self._answer(np.array([np.abs(self._stage(x)).max()]))

    # a table that depends on the model, cached per pointer
    def scaled(self, x, pointer):
        key = (pointer,) if self.flaw == "pointer" else (pointer, self.epoch)
        if self.table_key != key:
            self.table, self.table_key = 1.0 / (1.0 + self.psi), key
        return self._answer(x[:len(self.table)] * self.table[:len(x)])

    # a call that is refused after its work began
    def checked(self, x):
        self._stage(x)
        if not np.isfinite(x).all():
            self.stale = self.flaw == "refused"
            raise FakeError("refused: a non-finite element")
        return self._answer(np.cumsum(x))

    def _answer(self, out):
        if self.stale and self.last is not None and self.last.shape == out.shape:
            self.stale = False
            return self.last                      # the flaw: the result of the call before the refused one
        self.last = out
        return out


def _fake_probe(name, module, n, call, home=None):
    def build(rng, din, dout):
        return dict(x=rng.standard_normal(n if n else dout) + 2.0)

    return H.Probe(name, module, build, lambda eng, inp: dict(y=call(eng, inp["x"])), home)


FAKE_PROBES = {p.name: p for p in (
    _fake_probe("total.large", "total", 40, lambda e, x: e.total(x)), _fake_probe("total.small", "total", 7, lambda e, x: e.total(x)),
    _fake_probe("peak.large", "peak", 33, lambda e, x: e.peak(x)), _fake_probe("peak.small", "peak", 5, lambda e, x: e.peak(x)),
    _fake_probe("scaled.a", "scaled", 0, lambda e, x: e.scaled(x, 0x1000), "A"), _fake_probe("scaled.b", "scaled", 0, lambda e, x: e.scaled(x, 0x1000), "B"),
    _fake_probe("checked.small", "checked", 7, lambda e, x: e.checked(x)), _fake_probe("checked.large", "checked", 40, lambda e, x: e.checked(x)))}
FAKE_MODELS = {"A": (6, 1), "B": (6, 2), "C": (4, 3)}


def _fake_model(key):
    d, seed = FAKE_MODELS[key]
    rng = np.random.default_rng(seed)
    return rng.random(d), rng.standard_normal((d, d)), rng.random(d) + 0.1


def _fake_refuse(eng):
    x = np.ones(7)
    eng.checked(x)
    x[3] = np.nan
    with pytest.raises(FakeError):
        eng.checked(x)


FAKE_ROUTES = {"set_model.same": (lambda e: e.set_model(*_fake_model("B")), False), "set_model.smaller": (lambda e: e.set_model(*_fake_model("C")), False)}
FAKE_REFUSALS = {"checked.nan": (_fake_refuse, "checked.small", "total.small", None)}
FAMILY_RUNS = {
    "shrink_and_regrow": lambda h, e: h.shrink_and_regrow(e, {"large": "total.large", "small": "total.small"}),
    "neighbours": lambda h, e: h.neighbours(e, "total.large", "peak.small"),
    "routes": lambda h, e: h.route(e, "A", ["scaled.a"], FAKE_ROUTES["set_model.same"][0], ["scaled.a"]),
    "after_refusal": lambda h, e: h.after_refusal(e, None, _fake_refuse, "checked.small", "total.small"),
    "walk": lambda h, e: h.walk([e, FakeEngine(e.flaw)], H.walk_steps(0, 240, sorted(FAKE_PROBES), sorted(FAKE_ROUTES), sorted(FAKE_REFUSALS)),
                                FAKE_ROUTES, FAKE_REFUSALS, roaming=("scaled.a", "scaled.b"), square="A"),
}
# the flaw every family is there to find (the walk finds all three)
REJECTS = {"shrink_and_regrow": ["tail"], "neighbours": ["tail"], "routes": ["pointer"], "after_refusal": ["refused"],
           "walk": ["tail", "pointer", "refused"]}


def _harness():
    return H.Harness(lambda: FakeEngine(None), FAKE_PROBES, _fake_model)


@pytest.mark.parametrize("family", sorted(FAMILY_RUNS))
def test_every_family_accepts_the_honest_engine(family):
    h = _harness()
    FAMILY_RUNS[family](h, FakeEngine(None))
    assert h.fresh and h.log


@pytest.mark.parametrize("family,flaw", [(f, flaw) for f in sorted(REJECTS) for flaw in REJECTS[f]])
def test_every_family_rejects_a_flawed_engine(family, flaw):
    with pytest.raises(AssertionError, match="differs from the fresh handle's"):
        FAMILY_RUNS[family](_harness(), FakeEngine(flaw))


def test_control_on_the_fakes_and_the_comparison_itself():
    h = _harness()
    for name in FAKE_PROBES:
        eng = FakeEngine(None)
        if FAKE_PROBES[name].home:
            eng.set_model(*_fake_model(FAKE_PROBES[name].home))
        h.check_here(eng, name)
    a = dict(y=np.array([0.0, 1.0]))
    H.same_bits(a, dict(y=np.array([0.0, 1.0])))
    for other in (dict(y=np.array([-0.0, 1.0])), dict(y=np.array([0.0, 1.0], np.float32)), dict(y=np.array([[0.0, 1.0]])), dict(z=a["y"])):
        with pytest.raises(AssertionError):                          # a sign of zero, a dtype, a shape, a key
            H.same_bits(other, a)
    nan = np.array([np.nan])
    H.same_bits(dict(y=nan), dict(y=nan.copy()))                     # bits, not values: NaN equals NaN
