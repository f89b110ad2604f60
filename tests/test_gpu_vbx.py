"""GPU: the VBx resegmentation (csrc/vbx.hip) against its NumPy model (tests/vbx_model.py).

Parity runs a fixed number of iterations (epsilon = -inf, so that no stop decision can diverge) and compares gamma, pi and the
ELBO within 100 * max(d_ld, 2^-52 max|lp|) -- d_ld the model's own fp64-against-longdouble deviation, max|lp| the largest
|lp[t, s]| of the run (exp turns an absolute error of lp into a relative one of b); the ELBO relatively, with a floor of
2^-52 T.  Labels and n_clusters must EQUAL the model's (tests/test_vbx_model.py asserts the margins that make this
well-posed).  Measured on an MI355X (profiles/vbx_parity.json): the worst device deviation over the cases is 1.8e-14 on
gamma, 1.1e-14 on pi and 7.9e-15 relative on the ELBO, against bands of 1.4e-13 and more (2.2e-14 on the ELBO at T = 1,
where the device is exact); gamma and pi stay within 3 d_ld everywhere, the ELBO exceeds 10 d_ld once (200 x 33: 5.5e-15,
25 ulp of a sum of 200 logarithms taken in another order).

Every plda_vbx_dev call of this file goes through _run (the host forms are used where a wrapper is the subject): the inputs
sit between NaN (-1) neighbours, every output between guard bands filled with a payload that must stay intact outside the
output and be gone inside it (the pattern of tests/test_gpu_ahc.py)."""
import ctypes as C
import gc
import json
import os

import numpy as np
import pytest

import vbx_model as M

pytestmark = pytest.mark.gpu

GUARD = 16 << 10           # elements on either side
PAYLOAD = 0x7FC0DEAD
E_INVAL = -1
NEG_INF = float("-inf")


def _dev():
    import torch
    return torch.device("cuda", 0)


def _guarded_input(a):
    """a 1-D host array inside a device buffer whose neighbours are NaN (floats) or -1"""
    import torch
    t = torch.from_numpy(np.array(a, copy=True).ravel())
    buf = torch.empty(GUARD + t.numel() + GUARD, dtype=t.dtype, device=_dev())
    buf.fill_(float("nan") if t.dtype.is_floating_point else -1)
    body = buf[GUARD:GUARD + t.numel()]
    body.copy_(t.to(_dev()))
    return buf, body


class _Out:
    """a 1-D output of `count` elements between guard bands, everything pre-filled with the payload"""

    def __init__(self, count, dtype):
        import torch
        self.count = count
        self.words_per = torch.empty(0, dtype=dtype).element_size() // 4
        n = (GUARD + count + GUARD) * self.words_per
        self.words = torch.full((n,), PAYLOAD, dtype=torch.int32, device=_dev())
        self.body = self.words.view(dtype)[GUARD:GUARD + count]

    def ptr(self):
        return self.body.data_ptr() if self.count else self.words.view(self.body.dtype)[GUARD:].data_ptr()

    def check(self, what, written=True):
        w = self.words.cpu().numpy().reshape(-1, self.words_per)
        lo, hi = GUARD, GUARD + self.count
        assert (w[:lo] == np.int32(PAYLOAD)).all() and (w[hi:] == np.int32(PAYLOAD)).all(), "%s: guard band overwritten" % what
        inside = (w[lo:hi] == np.int32(PAYLOAD)).all(1)
        if written:
            assert int(inside.sum()) == 0, "%s: %d output elements never written" % (what, int(inside.sum()))
        else:
            assert inside.all(), "%s: written although the call failed or the output was not asked for" % what
        return self.body.cpu().numpy().copy()


def _lib():
    from plda_amd import _native as N
    return N.load()


def _model(d, seed=3, psi_scale=1.0):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    return rng.random(d), q * (0.5 + rng.random(d))[:, None], np.sort(rng.random(d) * 3.0 + 0.05)[::-1].copy() * psi_scale


def _engine():
    from plda_amd import MPlda
    e = MPlda(0)
    e.set_model(*_model(4))            # (VBx wants a fitted model even where Phi is given)
    return e


@pytest.fixture(scope="module")
def eng():
    return _engine()


def _run(eng, recs, phi, params=M.PARAMS["default"], max_iters=M.ITERS, epsilon=NEG_INF, sigma=5.0, posteriors=True, expect=0,
         offsets=None, gamma_short=0):
    """plda_vbx_dev on guarded buffers.  recs: [(y [T, D], labels [T])].  -> {"labels", "n_clusters", "gamma": [..], "pi": [..],
    "elbo" [R, max_iters], "iters"} (posteriors=False: the last four None), or the status code when expect != 0"""
    import torch
    from plda_amd import diarize
    d = recs[0][0].shape[1]
    y = np.concatenate([np.asarray(r[0], np.float64) for r in recs])
    lab = np.concatenate([np.asarray(r[1], np.int32) for r in recs])
    sizes = np.asarray([len(r[1]) for r in recs], np.int64)
    off = diarize.offsets_of(sizes) if offsets is None else np.asarray(offsets, np.int64)
    spk = np.asarray([max(1, min(64, int(np.max(r[1])) + 1)) for r in recs], np.int64)
    goff, poff = diarize.offsets_of(sizes * spk), diarize.offsets_of(spk)
    if gamma_short:
        goff[-1] -= gamma_short
    r, t = len(recs), int(sizes.sum())
    _, dy = _guarded_input(y)
    _, dl = _guarded_input(lab)
    _, dp = _guarded_input(np.asarray(phi, np.float64))
    oL, oK = _Out(t, torch.int32), _Out(r, torch.int32)
    oG, oP = _Out(int((sizes * spk).sum()), torch.float64), _Out(int(spk.sum()), torch.float64)
    oE, oI = _Out(r * max_iters, torch.float64), _Out(r, torch.int32)
    torch.cuda.synchronize()
    vp = lambda x: C.c_void_p(int(x)) if x else None
    hp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    fa, fb, p = params
    on = posteriors
    rc = _lib().plda_vbx_dev(eng._h, vp(dy.data_ptr()), d, vp(dp.data_ptr()), vp(dl.data_ptr()), hp(off), r, float(fa), float(fb),
                             float(p), float(sigma), int(max_iters), float(epsilon), vp(oL.ptr()), vp(oK.ptr()),
                             vp(oG.ptr()) if on else None, hp(goff) if on else None, vp(oP.ptr()) if on else None,
                             hp(poff) if on else None, vp(oE.ptr()) if on else None, vp(oI.ptr()) if on else None)
    torch.cuda.synchronize()
    assert rc == expect, "status %d: %s" % (rc, eng._lib.plda_last_error(eng._h).decode())
    outs = ((oL, "labels"), (oK, "n_clusters"), (oG, "gamma"), (oP, "pi"), (oE, "elbo"), (oI, "iters"))
    if expect:
        for o, name in outs:
            o.check(name, written=False)
        return rc
    res = {"labels": oL.check("labels"), "n_clusters": oK.check("n_clusters"), "gamma": None, "pi": None, "elbo": None, "iters": None}
    if not on:
        for o, name in outs[2:]:
            o.check(name, written=False)
        return res
    g, pi = oG.check("gamma"), oP.check("pi")
    res["gamma"] = [g[goff[q]:goff[q + 1]].reshape(int(sizes[q]), int(spk[q])) for q in range(r)]
    res["pi"] = [pi[poff[q]:poff[q + 1]] for q in range(r)]
    res["elbo"] = oE.check("elbo").reshape(r, max_iters)
    res["iters"] = oI.check("iters")
    return res


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _assert_same(got, want, what, rec=None, at=0):
    """bit equality of every output of recording `rec` of `got` (None: all) with recording `at` of `want`"""
    def pick(res, q):
        if q is None:
            return res
        return {k: (None if v is None else v[q]) for k, v in res.items() if k not in ("labels",)}
    a, b = pick(got, rec), pick(want, at if rec is not None else None)
    for k in a:
        if a[k] is None or b[k] is None:
            continue
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for x, y in zip(xs, ys):
            x, y = np.asarray(x), np.asarray(y)
            assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), "%s: %s differs" % (what, k)


# ------------------------------------------------------------------------------------------- plan
def test_plan_names_the_classes(eng):
    from plda_amd import diarize
    lo, hi = M.lds_boundary()
    assert diarize.vbx_plan(eng, lo, 8, 16) == {"cls": 0, "scratch_bytes": 0, "lds_doubles": M.LDS_DOUBLES}
    assert diarize.vbx_plan(eng, hi, 8, 16) == {"cls": 1, "scratch_bytes": 8 * M.state_doubles(hi, 8, 16), "lds_doubles": M.LDS_DOUBLES}
    assert diarize.vbx_plan(eng, 4096, 64, 128)["scratch_bytes"] == 8 * M.state_doubles(4096, 64, 128)
    out = (C.c_int32 * 3)()
    for t, s, d in ((0, 1, 1), (4097, 1, 1), (1, 0, 1), (1, 65, 1), (1, 1, 0)):
        assert _lib().plda_vbx_plan(eng._h, t, s, d, out) == E_INVAL


# ------------------------------------------------------------------------------------------- parity
_PARITY = {}


def _parity_figures(got, want, ld, t, q=0):
    """the deviations of recording q of a device run of ITERS iterations from the model's fp64 run `want`, the model's own
    fp64-against-longdouble deviations d_ld, and the bands: 100 * max(d_ld, 2^-52 max|lp|) on gamma and pi, 100 * max(d_ld,
    2^-52 T) on the ELBO, relatively"""
    d_gamma, d_pi, d_elbo = M.deviation(want, ld)
    floor = 2.0 ** -52 * want["max_lp"]
    dev_gamma = float(np.max(np.abs(got["gamma"][q] - want["gamma"])))
    dev_pi = float(np.max(np.abs(got["pi"][q] - want["pi"])))
    dev_elbo = float(np.max(np.abs(got["elbo"][q] - want["elbo"]) / np.abs(want["elbo"])))
    fig = {"iters": M.ITERS, "max_abs_lp": want["max_lp"],
           "d_ld": {"gamma": d_gamma, "pi": d_pi, "elbo_rel": d_elbo},
           "device": {"gamma": dev_gamma, "pi": dev_pi, "elbo_rel": dev_elbo},
           "band": {"gamma": 100 * max(d_gamma, floor), "pi": 100 * max(d_pi, floor), "elbo_rel": 100 * max(d_elbo, 2.0 ** -52 * t)}}
    return fig


def _assert_parity(got, want, ld, t, q=0, fig=None):
    """the parity rule on recording q: ITERS iterations; gamma, pi and the ELBO within the bands of _parity_figures; labels and
    n_clusters EQUAL to the model's.  Returns the figures."""
    fig = fig or _parity_figures(got, want, ld, t, q)
    assert int(got["iters"][q]) == M.ITERS
    for key in ("gamma", "pi", "elbo_rel"):
        assert fig["device"][key] <= fig["band"][key], (key, fig)
    if len(got["gamma"]) == 1:                                    # one recording: the whole arrays, their lengths included
        assert got["iters"].tolist() == [M.ITERS]
        assert np.array_equal(got["labels"], want["labels"]) and got["n_clusters"].tolist() == [want["n_clusters"]]
    off = int(sum(g.shape[0] for g in got["gamma"][:q]))
    assert np.array_equal(got["labels"][off:off + len(want["labels"])], want["labels"]) and int(got["n_clusters"][q]) == want["n_clusters"]
    return fig


@pytest.mark.parametrize("name", list(M.cases()))
def test_parity_with_the_model(eng, name):
    t, d, k, s, _ = M.cases()[name]
    ref = M.reference(name)
    want, ld = ref["f64"], ref["ld"]
    got = _run(eng, [(ref["y"], ref["labels"])], ref["phi"], ref["params"])
    fig = _parity_figures(got, want, ld, t)
    fig.update({"T": t, "D": d, "K": k, "S": s, "params": list(ref["params"])})
    print("vbx parity %s: %s" % (name, json.dumps(fig)))
    _PARITY[name] = fig
    path = os.environ.get("VBX_PARITY_JSON")
    if path:                                                    # (scripts/vbx_bench.py --parity collects the figures)
        with open(path, "w") as f:
            json.dump(_PARITY, f, indent=1, sort_keys=True)
    _assert_parity(got, want, ld, t, fig=fig)
    assert plan_class(eng, t, s, d) == (1 if M.state_doubles(t, s, d) > M.LDS_DOUBLES else 0)


def plan_class(eng, t, s, d):
    from plda_amd import diarize
    return diarize.vbx_plan(eng, t, s, d)["cls"]


# ------------------------------------------------------------------------------------------- stop rule
@pytest.mark.parametrize("name", M.STOP_CASES)
def test_stop_rule(eng, name):
    ref = M.reference(name)
    eps, want = M.stop_epsilon(ref)
    got = _run(eng, [(ref["y"], ref["labels"])], ref["phi"], ref["params"], epsilon=eps)
    n = want["iters"]
    assert got["iters"].tolist() == [n]
    assert np.isfinite(got["elbo"][0][:n]).all() and np.isnan(got["elbo"][0][n:]).all()
    assert np.array_equal(got["labels"], want["labels"]) and got["n_clusters"].tolist() == [want["n_clusters"]]


def test_max_iters_one_runs_one_iteration(eng):
    ref = M.reference("130x7x3x5")
    got = _run(eng, [(ref["y"], ref["labels"])], ref["phi"], ref["params"], max_iters=1, epsilon=1e300)
    assert got["iters"].tolist() == [1] and np.isfinite(got["elbo"]).all() and got["elbo"].shape == (1, 1)
    fa, fb, p = ref["params"]
    want = M.run(ref["y"], ref["labels"], ref["phi"], fa, fb, p, max_iters=1)
    assert np.array_equal(got["labels"], want["labels"])
    assert abs(got["elbo"][0, 0] - want["elbo"][0]) <= 1e-10 * abs(want["elbo"][0])


# ------------------------------------------------------------------------------------------- determinism, on the bits
D_MIX = 16


def _mixed():
    """recordings of one dimension in both storage classes, (1, S = 1) and a full wave of speakers among them"""
    lo, hi = M.lds_boundary(D_MIX, 8)
    shapes = [(40, 2, 3), (hi, 4, 8), (1, 1, 1), (65, 3, 64), (lo, 4, 8), (300, 4, 10), (900, 3, 7), (2, 1, 2), (4096, 4, 8)]
    recs = []
    for q, (t, k, s) in enumerate(shapes):
        y, labels, _, phi = M.generate(t, D_MIX, k, s, 500 + q)
        recs.append((y, labels))
    return recs, phi


@pytest.fixture(scope="module")
def mixed(eng):
    recs, phi = _mixed()
    classes = [plan_class(eng, len(l), int(l.max()) + 1, D_MIX) for _, l in recs]
    assert 0 in classes and 1 in classes
    return recs, phi, _run(eng, recs, phi, M.PARAMS["unit"], max_iters=6)


def test_same_call_twice(eng, mixed):
    recs, phi, first = mixed
    _assert_same(_run(eng, recs, phi, M.PARAMS["unit"], max_iters=6), first, "second call")


def test_alone_equals_inside_a_batch(eng, mixed):
    recs, phi, batch = mixed
    off = np.concatenate([[0], np.cumsum([len(l) for _, l in recs])])
    for q, rec in enumerate(recs):
        one = _run(eng, [rec], phi, M.PARAMS["unit"], max_iters=6)
        _assert_same(batch, one, "recording %d" % q, rec=q)
        assert np.array_equal(batch["labels"][off[q]:off[q + 1]], one["labels"])


def _budget_engine(monkeypatch, budget=None, poison=False):
    if budget:
        monkeypatch.setenv("PLDA_VBX_SCRATCH_BYTES", str(budget))
    if poison:
        monkeypatch.setenv("PLDA_SCRATCH_POISON", "1")
    e = _engine()
    monkeypatch.delenv("PLDA_VBX_SCRATCH_BYTES", raising=False)
    monkeypatch.delenv("PLDA_SCRATCH_POISON", raising=False)
    return e


def test_small_budget_equals_default(monkeypatch, mixed):
    """1 MiB does not hold the scratch of the three HBM-class recordings (156 + 175 + 887 KB): two launches instead of one"""
    recs, phi, first = mixed
    small = _budget_engine(monkeypatch, 1 << 20)
    held = _lib().plda_device_bytes_held()
    _assert_same(_run(small, recs, phi, M.PARAMS["unit"], max_iters=6), first, "1 MiB budget")
    assert _lib().plda_device_bytes_held() - held < (2 << 20)


def test_poisoned_scratch_equals_fresh(monkeypatch, mixed):
    from plda_amd import MPlda
    recs, phi, first = mixed
    e = _budget_engine(monkeypatch, poison=True)
    got = _run(e, recs, phi, M.PARAMS["unit"], max_iters=6)
    e.synchronize()
    del e
    MPlda(0)                           # the switch off again for whatever runs next in this process
    _assert_same(got, first, "poisoned scratch")


def test_labels_without_the_nullable_outputs(eng, mixed):
    recs, phi, first = mixed
    got = _run(eng, recs, phi, M.PARAMS["unit"], max_iters=6, posteriors=False)
    assert np.array_equal(got["labels"], first["labels"]) and np.array_equal(got["n_clusters"], first["n_clusters"])


def test_create_vbx_destroy_gives_back_every_byte():
    from plda_amd import diarize
    recs, phi = _mixed()
    recs = recs[:3]
    y, lab = np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs])
    off = diarize.offsets_of([len(r[1]) for r in recs])
    gc.collect()
    first = _lib().plda_device_bytes_held()
    for cycle in range(10):
        e = _engine()
        diarize.vbx(e, y, off, lab, phi, max_iters=3, return_posteriors=bool(cycle % 2))
        assert _lib().plda_device_bytes_held() > first
        del e
        gc.collect()
        held = _lib().plda_device_bytes_held()
        assert held == first, "cycle %d: %d bytes of device memory not given back" % (cycle, held - first)


# ------------------------------------------------------------------------------------------- errors
def _two():
    a = M.generate(30, 8, 2, 4, 1)
    b = M.generate(50, 8, 2, 3, 2)
    return [(a[0].copy(), a[1].copy()), (b[0].copy(), b[1].copy())], a[3]


def _fails(eng, recs, phi, text=None, **kw):
    assert _run(eng, recs, phi, expect=E_INVAL, **kw) == E_INVAL
    if text:
        assert text in eng._lib.plda_last_error(eng._h).decode()
    good, gphi = _two()                                    # the handle works on
    assert _run(eng, good, gphi, max_iters=2)["iters"].tolist() == [2, 2]


def test_error_nan_row(eng):
    recs, phi = _two()
    recs[1][0][7, :] = np.nan
    _fails(eng, recs, phi, "8 non-finite")


def test_error_label_64(eng):
    recs, phi = _two()
    recs[0][1][3] = 64
    _fails(eng, recs, phi, "1 labels outside")


def test_error_label_minus_one(eng):
    recs, phi = _two()
    recs[1][1][0] = -1
    _fails(eng, recs, phi, "1 labels outside")


def test_error_bad_offsets(eng):
    recs, phi = _two()
    _fails(eng, recs, phi, offsets=[1, 30, 80])
    _fails(eng, recs, phi, offsets=[0, 30, 30])
    _fails(eng, recs, phi, offsets=[0, 50, 30])


def test_error_recording_of_4097(eng):
    y = np.zeros((4097, 2))
    _fails(eng, [(y, np.zeros(4097, np.int32))], np.ones(2), "PLDA_AHC_MAX")


def test_error_fa_zero(eng):
    recs, phi = _two()
    _fails(eng, recs, phi, "Fa", params=(0.0, 17.0, 0.99))


def test_error_loop_prob_one(eng):
    recs, phi = _two()
    _fails(eng, recs, phi, "loop_prob", params=(0.3, 17.0, 1.0))


def test_error_short_gamma_interval(eng):
    recs, phi = _two()
    _fails(eng, recs, phi, "gamma interval 1", gamma_short=1)


def test_error_negative_phi_and_unfitted(eng):
    from plda_amd import MPlda
    recs, phi = _two()
    bad = phi.copy()
    bad[2] = -1.0
    _fails(eng, recs, bad, "1 entries of Phi")
    assert _run(MPlda(0), recs, phi, expect=-4) == -4       # PLDA_E_NOT_FITTED


# ------------------------------------------------------------------------------------------- the model's space, the wrappers
def test_project_rows_against_numpy():
    from plda_amd import MPlda
    e = MPlda(0)
    mean, T, psi = _model(40, 11)
    e.set_model(mean, T, psi)
    rng = np.random.default_rng(4)
    x = rng.standard_normal((77, 40)) + mean
    for dout in (40, 24):
        if dout < 40:
            e.truncate(dout)
        m = e.get_model()
        want = x @ m["transform"].T + m["offset"]
        got = e.project_rows(x)
        assert got.shape == (77, dout)
        assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, float(np.max(np.abs(want))))
    with pytest.raises(Exception):
        e.project_rows(x[:, :39])


def _planted(mean, T, psi, t, k, seed):
    """rows from the model's own generative form, a sticky speaker sequence -> (x [t, Din], speaker of each row)"""
    rng = np.random.default_rng(seed)
    d = len(psi)
    spk = np.empty(t, np.int64)
    cur = 0
    for i in range(t):
        if i and rng.random() >= 0.95:
            cur = int(rng.integers(k))
        spk[i] = cur
    u = (rng.standard_normal((k, d)) * np.sqrt(psi))[spk] + rng.standard_normal((t, d))
    m = {"transform": T, "mean": mean}
    return mean + u @ np.linalg.inv(m["transform"]).T, spk


def test_resegment_and_diarize():
    """resegment == vbx on the projected rows, bit for bit; diarize == cluster then resegment; on planted three-speaker
    recordings whose AHC stops early at six clusters (over-split) diarize returns the planted partition"""
    from liblda.plda import PLDA
    from plda_amd import diarize
    d = 24
    mean, T, psi = _model(d, 77, psi_scale=8.0)
    p = PLDA(0)
    e = p._instance
    e.set_model(mean, T, psi)
    rows, spk = zip(*[_planted(mean, T, psi, 150, 3, 900 + q) for q in range(4)])
    x, off = np.concatenate(rows), diarize.offsets_of([150] * 4)
    ahc_labels, ahc_k = p.cluster(x, off, threshold=None, num_speakers=6)
    assert ahc_k.tolist() == [6] * 4
    a = e.resegment(x, off, ahc_labels, return_posteriors=True)
    b = diarize.vbx(e, e.project_rows(x), off, ahc_labels, return_posteriors=True)
    _assert_same({"l": a[0], "k": a[1], **a[2]}, {"l": b[0], "k": b[1], **b[2]}, "resegment against vbx")
    c = p.diarize(x, off, threshold=None, num_speakers=6)
    assert np.array_equal(c[0], a[0]) and np.array_equal(c[1], a[1])
    c = p.resegment(x, off, ahc_labels)
    assert np.array_equal(c[0], a[0]) and np.array_equal(c[1], a[1])
    for q in range(4):
        want, k = M.first_member_labels(spk[q])
        assert a[1][q] == k == 3
        assert np.array_equal(a[0][off[q]:off[q + 1]], want), "recording %d" % q
    # the host form against the model, on the projected rows and the model's psi
    y = e.project_rows(x)
    want = M.run(y[:150], ahc_labels[:150], e.get_model()["psi"])
    assert np.array_equal(a[0][:150], want["labels"]) and a[2]["iters"][0] == want["iters"]
    assert np.max(np.abs(a[2]["gamma"][0] - want["gamma"])) <= 1e-9
    with pytest.raises(ValueError, match="loop_prob"):
        e.resegment(x, off, ahc_labels, loop_prob=1.0)
