"""GPU: multi-system score fusion by logistic regression (csrc/fusion.hip; include/plda_hip.h "multi-system score fusion"),
every call through the C ABI, against the host model tests/fusion_model.py.

  1. the pass record against the model for K in {1, 2, 3, 8} over shapes chosen for the kernel's paths (one row, one column, a
     ragged last strip, more than one strip and slice; tall matrices whose workgroups walk 5 or 6 rows: full and partial
     steps of every U, runs of up to 256 * 6 sequential additions -- inside the header's WORST-case band, not only its typical
     one), per-system pitches and alignments, four points and three label
     layouts: integers, fp32 extremes exactly; each sum within 1e-12 * sum|term| (derived in the header, valid where
     (K + 1) Ymax <= 2000, which every case asserts); ymin / ymax within (K + 1) Ymax 2^-52; the same call twice bit-identical;
  2. K = 1 against the calibration pass (K10) on the same matrix;
  3. lists against matrices;
  4. the fit: optimality by the MODEL's gradient and Hessian, Cllr against the best single calibrated system, pass count,
     a separable set, the refusals by name;
  5. plda_fusion_map_dev bit for bit against the Fraction chain, in place, guard columns;
  6. liblda.PLDA.fuse / score_matrix_fused end to end;
  7. guard bands, poisoned scratch, create / fuse / destroy, API edges.

Run with -s to see the measured figures next to each bound.  Nothing here provokes a fault."""
import ctypes as C
import warnings

import numpy as np
import pytest

import calibration_model as cm
import fusion_model as fm

pytestmark = pytest.mark.gpu

ENV = ("PLDA_SCRATCH_POISON",)
BOUND = 1e-12
INTS = ("K", "Np", "Nn", "miss", "fa", "nonfinite")


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _engine(monkeypatch, poison=False):
    from plda_amd import MPlda
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    if poison:
        monkeypatch.setenv("PLDA_SCRATCH_POISON", "1")
    eng = MPlda(0)
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    return eng


def _labels(rng, m, nt, layout):
    """random: a dozen speakers; sparse: 4000 speakers, so most waves of 64 lanes x 4 columns hold no target; blocks: runs of
    rows and of 512 columns with one speaker, so whole waves are targets."""
    if layout == "blocks":
        es, ts = (np.arange(m) // 7) % 3, (np.arange(nt) // 512) % 3
    else:
        k = 4000 if layout == "sparse" else 12
        es, ts = rng.integers(0, k, m), rng.integers(0, k, nt)
    es[0] = ts[0] = 0                       # at least one target ...
    if nt > 1:
        ts[-1] = 5000                       # ... and one non-target (a speaker nobody enrolled)
    else:
        es[-1] = 5000
    return es.astype(np.int64), ts.astype(np.int64)


def _systems(rng, m, nt, k, tgt):
    """K correlated systems on one trial set: a common part (targets 4 higher) in each system's own units plus its own noise."""
    base = rng.standard_normal((m, nt)) * 3.0 + 4.0 * tgt
    unit = [1.0, 2.5, 0.4, 1.0, 1.5, 0.7, 2.0, 1.2]
    return [(unit[j] * (base + rng.standard_normal((m, nt))) - 0.5 * j).astype(np.float32) for j in range(k)]


class Placed(object):
    """K host matrices placed on the device, each in its own allocation with its own pitch and base offset (floats), between
    guard floats that no call may change."""
    G = 64
    SENTINEL = np.float32(-7.25e30)

    def __init__(self, S, lds, offs):
        self.S, self.lds, self.offs = S, lds, offs
        self.m, self.nt = S[0].shape
        self.host, self.dev = [], []
        for s, ld, off in zip(S, lds, offs):
            flat = np.full(self.G + off + self.m * ld + self.G, self.SENTINEL, np.float32)
            body = flat[self.G + off:self.G + off + self.m * ld].reshape(self.m, ld)
            body[:, :self.nt] = s
            self.host.append(flat)
            self.dev.append(_t(flat))
        assert all(d.data_ptr() % 16 == 0 for d in self.dev)            # so that `off` alone decides the alignment

    @property
    def ptrs(self):
        return [d.data_ptr() + 4 * (self.G + off) for d, off in zip(self.dev, self.offs)]

    def unchanged(self):
        return all(np.array_equal(d.cpu().numpy().view(np.int32), h.view(np.int32)) for d, h in zip(self.dev, self.host))


def _placement(k, nt, mode):
    """Pitches differ per system (ld = Nt for system 0, a multiple of 4 above Nt for the next, Nt + 1 ..); mode none: every base
    16-byte aligned; one: the LAST system's base is one float off; all: every base is."""
    up4 = (nt + 3) // 4 * 4
    lds = [nt, up4 + 4, nt + 1, up4, nt, up4 + 8, nt + 3, up4 + 4][:k]
    offs = {"none": [0] * k, "one": [0] * (k - 1) + [1], "all": [1] * k}[mode]
    return lds, offs


def _theta(S, a, c):
    """The midpoint of two adjacent model chain values at least 1e-9 apart, near the median: the device's y may differ from
    the model's in the last bit ((K + 1) Ymax 2^-52 < 5e-13 here), so no trial changes sides and miss / fa are exact."""
    ys = np.unique(fm.chain([s.ravel() for s in S], a, c))
    if ys.shape[0] == 1:
        return float(ys[0]) - 0.5           # every y is c itself (a = 0): any threshold away from it
    i = (ys.shape[0] - 1) // 2
    gaps = np.nonzero(np.diff(ys[i:]) >= 1e-9)[0]
    assert gaps.size, "no two adjacent chain values 1e-9 apart"
    lo, hi = ys[i + gaps[0]], ys[i + gaps[0] + 1]
    assert hi - lo >= 1e-9
    return float(lo + (hi - lo) / 2)


def _compare(what, got, ref):
    k = ref["K"]
    assert (k + 1) * ref["Ymax"] <= 2000.0, (what, ref["Ymax"])       # where the header's 1e-12 band holds
    for key in INTS:
        assert got[key] == ref[key], (what, key, got[key], ref[key])
    assert np.array_equal(got["smin"], ref["smin"]) and np.array_equal(got["smax"], ref["smax"]), what
    ytol = (k + 1) * ref["Ymax"] * 2.0 ** -52
    for key in ("ymin_t", "ymax_t", "ymin_n", "ymax_n"):
        assert abs(got[key] - ref[key]) <= ytol, (what, key, got[key], ref[key])
    worst = 0.0
    for cls in ("t", "n"):
        for name in ("L_", "G_", "H_"):
            g, r, s = (np.atleast_1d(np.asarray(x[name + cls], np.float64)) for x in (got, ref, ref["abs"]))
            assert g.shape == r.shape, (what, name + cls)
            err = np.abs(g - r)
            assert np.all(err[s == 0.0] == 0.0), (what, name + cls)
            if np.any(s > 0):
                worst = max(worst, float((err[s > 0] / s[s > 0]).max()))
            assert np.all(err <= BOUND * s), (what, name + cls, g, r, err / np.maximum(s, 1e-300))
    print("%s: max |sum - model| / sum|term| = %.3g (bound %.0e)" % (what, worst, BOUND))


def _same_bits(x, y):
    assert x.keys() == y.keys()
    for key in x:
        assert np.asarray(x[key]).tobytes() == np.asarray(y[key]).tobytes(), key


def _points(S, tgt, k, which):
    """(a, c): the start; one system alone; a fitted point; a cancelling point (1, -1, ..) on the correlated systems."""
    pos, neg = [s[tgt] for s in S], [s[~tgt] for s in S]
    out = {"start": (np.zeros(k), 0.0), "alone": (np.eye(k)[k - 1], -0.25)}
    if "fitted" in which and pos[0].shape[0] >= 50 and neg[0].shape[0] >= 50:      # (a handful of targets would be separable)
        f = fm.fit([p[:3000] for p in pos], [n[:20000] for n in neg], 0.3)
        out["fitted"] = (f["a"], f["b"] + fm.logit(0.3))
    out["cancel"] = (np.array([(-1.0) ** j for j in range(k)]) * np.array([1.0, 0.4, 2.5, 1.0, 1 / 1.5, 1 / 0.7, 0.5, 1 / 1.2][:k]), 0.125)
    return [(n, out[n]) for n in which if n in out]


# ------------------------------------------------------------------------------------------- 1. the pass record
SHAPES = [(300, 500), (37, 1023), (1, 2000), (700, 1), (5, 4099), (513, 1025)]
CASES = [(m, nt, k, ("none", "one", "all")[(i + j) % 3], ("random", "sparse", "blocks")[(i + 2 * j) % 3])
         for i, (m, nt) in enumerate(SHAPES) for j, k in enumerate((1, 2, 3, 8))]
CASES += [(300, 500, 3, "all", "random"), (300, 500, 8, "one", "blocks"), (513, 1025, 2, "all", "sparse")]


@pytest.mark.parametrize("m,nt,k,mode,layout", CASES)
def test_pass_record_matches_the_model(monkeypatch, m, nt, k, mode, layout):
    from plda_amd import fusion as FU
    eng = _engine(monkeypatch)
    rng = np.random.default_rng(m * 7919 + nt * 31 + k)
    es, ts = _labels(rng, m, nt, layout)
    tgt = es[:, None] == ts[None, :]
    S = _systems(rng, m, nt, k, tgt)
    P = Placed(S, *_placement(k, nt, mode))
    des, dts = _t(es), _t(ts)
    for name, (a, c) in _points(S, tgt, k, ("start", "alone", "fitted", "cancel")):
        theta = _theta(S, a, c)
        got = FU.pass_from_matrices_dev(eng, P.ptrs, P.lds, m, nt, des.data_ptr(), dts.data_ptr(), a, c, theta)
        again = FU.pass_from_matrices_dev(eng, P.ptrs, P.lds, m, nt, des.data_ptr(), dts.data_ptr(), a, c, theta)
        _same_bits(got, again)
        ref = fm.pass_matrices(S, es, ts, a, c, theta)
        _compare("%dx%d K %d %s %s at %s" % (m, nt, k, mode, layout, name), got, ref)
        assert got["Np"] == int(tgt.sum()) and got["Np"] + got["Nn"] == m * nt
    assert P.unchanged()


# A workgroup walks rows_per_wg = ceil(M / min(M, 4096 / strips)) rows in steps of U = 4 (K <= 2), 2 (K <= 4) or 1 rows.  Every
# shape above has rows_per_wg = 1; these have one strip and 5 or 6 rows per workgroup -- a full step and a partial one for
# every U -- and a last workgroup of one row (17001 = 5 * 3400 + 1; 20485 = 6 * 3414 + 1).
TALL = [(17001, 130, 1, "none", "blocks"), (17001, 130, 2, "one", "sparse"), (17001, 70, 4, "one", "blocks"), (17001, 70, 3, "all", "sparse"),
        (17001, 66, 8, "one", "blocks"), (17001, 66, 8, "none", "sparse"), (20485, 66, 1, "all", "sparse")]


@pytest.mark.parametrize("m,nt,k,mode,layout", TALL)
def test_pass_record_several_rows_per_workgroup(monkeypatch, m, nt, k, mode, layout):
    from plda_amd import fusion as FU
    slices = min(m, 4096)
    rpw = -(-m // slices)
    u = 4 if k <= 2 else 2 if k <= 4 else 1
    assert rpw in (5, 6) and (u == 1 or rpw % u != 0)                     # full steps and a partial last one where U > 1
    eng = _engine(monkeypatch)
    rng = np.random.default_rng(m + nt * 31 + k)
    es, ts = _labels(rng, m, nt, layout)
    if layout == "sparse":
        es[::97] = ts[3]                        # a few dozen targets spread over the workgroups, most waves without one
    tgt = es[:, None] == ts[None, :]
    S = _systems(rng, m, nt, k, tgt)
    P = Placed(S, *_placement(k, nt, mode))
    des, dts = _t(es), _t(ts)
    for name, (a, c) in _points(S, tgt, k, ("cancel",)):
        theta = _theta(S, a, c)
        got = FU.pass_from_matrices_dev(eng, P.ptrs, P.lds, m, nt, des.data_ptr(), dts.data_ptr(), a, c, theta)
        _same_bits(got, FU.pass_from_matrices_dev(eng, P.ptrs, P.lds, m, nt, des.data_ptr(), dts.data_ptr(), a, c, theta))
        _compare("%dx%d K %d %s %s (%d rows per workgroup) at %s" % (m, nt, k, mode, layout, rpw, name), got,
                 fm.pass_matrices(S, es, ts, a, c, theta))
        assert got["Np"] == int(tgt.sum()) and got["Np"] + got["Nn"] == m * nt
    assert P.unchanged()


def test_pass_record_2048x4096_three_systems(monkeypatch):
    """More than one row slice per strip and four strips; 16 blocks' partials through the reduce."""
    from plda_amd import fusion as FU
    eng = _engine(monkeypatch)
    m, nt, k = 2048, 4096, 3
    rng = np.random.default_rng(77)
    es, ts = _labels(rng, m, nt, "random")
    es[:], ts[:-1] = np.arange(m) // 8, np.arange(nt - 1) // 16              # 8 / 16 utterances per speaker: 0.4 % targets
    tgt = es[:, None] == ts[None, :]
    S = _systems(rng, m, nt, k, tgt)
    P = Placed(S, [nt, nt + 4, nt], [0, 0, 1])
    des, dts = _t(es), _t(ts)
    for name, (a, c) in _points(S, tgt, k, ("cancel",)):                     # (the host model takes ten seconds per point here)
        theta = _theta(S, a, c)
        got = FU.pass_from_matrices_dev(eng, P.ptrs, P.lds, m, nt, des.data_ptr(), dts.data_ptr(), a, c, theta)
        _same_bits(got, FU.pass_from_matrices_dev(eng, P.ptrs, P.lds, m, nt, des.data_ptr(), dts.data_ptr(), a, c, theta))
        _compare("2048x4096 K 3 at %s" % name, got, fm.pass_matrices(S, es, ts, a, c, theta))


# ------------------------------------------------------------------------------------------- 2. K = 1 against K10
@pytest.mark.parametrize("m,nt,ld,off", [(300, 500, 500, 0), (513, 1025, 1028, 1)])
def test_k1_agrees_with_the_calibration_pass(monkeypatch, m, nt, ld, off):
    """At a = 1, c = 0 the chain value is the score itself, so the counts (taken on y here, on s there) and the extremes agree
    exactly.  The sums are each held to the band of the model, hence to twice the band of each other; they are NOT the same
    bits, in either class: the targets are added per thread and tree there, in lane order per wave here; the non-target G1,
    H1, H2 are accumulated as fma(g, s, acc) / fma(w s, s, acc) here and as a rounded product plus an addition there; and the
    partial records of the blocks are added by different trees (256 running sums there, 8 here), which reaches L, G0 and H0
    too as soon as there is more than one block."""
    from plda_amd import calibration as CB, fusion as FU
    eng = _engine(monkeypatch)
    rng = np.random.default_rng(m + nt)
    es, ts = _labels(rng, m, nt, "random")
    tgt = es[:, None] == ts[None, :]
    S = _systems(rng, m, nt, 1, tgt)
    P = Placed(S, [ld], [off])
    des, dts = _t(es), _t(ts)
    theta = _theta(S, [1.0], 0.0)
    got = FU.pass_from_matrices_dev(eng, P.ptrs, P.lds, m, nt, des.data_ptr(), dts.data_ptr(), [1.0], 0.0, theta)
    k10 = CB.pass_from_matrix_dev(eng, P.ptrs[0], ld, m, nt, des.data_ptr(), dts.data_ptr(), 1.0, 0.0, theta)
    ref = fm.pass_matrices(S, es, ts, [1.0], 0.0, theta)
    _compare("K = 1 at the identity", got, ref)
    for key in ("Np", "Nn", "miss", "fa", "nonfinite"):
        assert got[key] == k10[key], key
    assert got["smin"][0] == min(k10["min_t"], k10["min_n"]) and got["smax"][0] == max(k10["max_t"], k10["max_n"])
    assert got["ymin_t"] == float(k10["min_t"]) and got["ymax_n"] == float(k10["max_n"])
    for cls in ("t", "n"):
        mine = [got["L_" + cls], got["G_" + cls][0], got["G_" + cls][1], got["H_" + cls][0], got["H_" + cls][1], got["H_" + cls][2]]
        scale = [ref["abs"]["L_" + cls]] + list(ref["abs"]["G_" + cls]) + list(ref["abs"]["H_" + cls])
        model = [ref["L_" + cls]] + list(ref["G_" + cls]) + list(ref["H_" + cls])
        for x, name, s, r in zip(mine, cm.SUMS, scale, model):
            assert abs(k10[name + "_" + cls] - r) <= BOUND * s and abs(x - k10[name + "_" + cls]) <= 2 * BOUND * s, (name, cls)


# ------------------------------------------------------------------------------------------- 3. lists against matrices
@pytest.mark.parametrize("k", [1, 3, 8])
def test_lists_agree_with_matrices_and_are_deterministic(monkeypatch, k):
    from plda_amd import fusion as FU
    eng = _engine(monkeypatch)
    m, nt = 301, 777
    rng = np.random.default_rng(40 + k)
    es, ts = _labels(rng, m, nt, "random")
    tgt = es[:, None] == ts[None, :]
    S = _systems(rng, m, nt, k, tgt)
    P = Placed(S, *_placement(k, nt, "one"))
    des, dts = _t(es), _t(ts)
    pos, neg = fm.split(S, es, ts)
    for name, (a, c) in _points(S, tgt, k, ("alone", "fitted")):
        theta = _theta(S, a, c)
        ref = fm.pass_record(pos, neg, a, c, theta)
        mat = FU.pass_from_matrices_dev(eng, P.ptrs, P.lds, m, nt, des.data_ptr(), dts.data_ptr(), a, c, theta)
        lst = FU.pass_from_lists(eng, pos, neg, a, c, theta)
        _same_bits(lst, FU.pass_from_lists(eng, pos, neg, a, c, theta))
        _compare("K %d matrix at %s" % (k, name), mat, ref)
        _compare("K %d lists at %s" % (k, name), lst, ref)
        for key in INTS:
            assert lst[key] == mat[key]
    # one trial per class, and more trials than one grid pass of 4096 x 256 threads covers
    p1, n1, w = [p[:1] for p in pos], [n[:1] for n in neg], np.ones(k) * 0.1
    theta = _theta([np.concatenate(x) for x in zip(p1, n1)], w, 0.0)
    _compare("one + one", FU.pass_from_lists(eng, p1, n1, w, 0.0, theta), fm.pass_record(p1, n1, w, 0.0, theta))
    if k == 3:
        big = [np.tile(n, 6)[:1_100_000] for n in neg]
        a = np.array([0.2, -0.1, 0.3])
        theta = _theta([np.concatenate(x) for x in zip(pos, neg)], a, 0.1)
        _compare("lists 1.1e6", FU.pass_from_lists(eng, pos, big, a, 0.1, theta), fm.pass_record(pos, big, a, 0.1, theta))


# ------------------------------------------------------------------------------------------- 4. the fit
def _fit_case(rng, m, nt, k):
    es, ts = _labels(rng, m, nt, "random")
    tgt = es[:, None] == ts[None, :]
    base = rng.standard_normal((m, nt)) * 2.0 + 2.5 * tgt - 1.0
    unit, shift = [1.0, 150.0, 0.5, 1.0], [0.0, 0.0, 0.0, -20.0]         # LLRs of a few hundred; log-posteriors around -20
    S = [(unit[j] * (base + 1.5 * rng.standard_normal((m, nt))) + shift[j]).astype(np.float32) for j in range(k)]
    return es, ts, tgt, S


def _assert_fit_is_optimal(f, pos, neg, k, prior):
    """the optimality rule: the MODEL's own lambda2 at the device's (a, b) is at most 1e-17 (10 x the fit's tolerance); Cllr
    after within BOUND of the model's; the pass count.  Returns lambda2."""
    rec = fm.pass_record(pos, neg, f.a, f.b + fm.logit(prior))
    assert (k + 1) * rec["Ymax"] <= 2000.0
    lam2 = fm.newton(rec, prior)[2]
    assert f.converged and not f.separable and f.n_systems == k and f.prior == prior
    assert lam2 <= 1e-17, lam2
    after = fm.pass_record(pos, neg, f.a, f.b)
    scale = 0.5 / after["Np"] * after["abs"]["L_t"] + 0.5 / after["Nn"] * after["abs"]["L_n"]
    assert abs(f.cllr_after * fm.LN2 - fm.objective(after, 0.5)) <= BOUND * scale
    # one pass at the start, one per trial point (at least one per iteration), one more for cllr_after off prior 0.5
    assert 1 + f.iterations + (prior != 0.5) <= f.passes <= 100 + 30 + 2
    return lam2


@pytest.mark.parametrize("prior", [0.5, 0.05])
@pytest.mark.parametrize("k", [2, 4])
def test_fit_is_optimal_by_the_models_own_derivatives(monkeypatch, k, prior):
    from plda_amd import calibration as CB, fusion as FU
    eng = _engine(monkeypatch)
    rng = np.random.default_rng(41 + k)
    m, nt = 300, 900
    es, ts, tgt, S = _fit_case(rng, m, nt, k)
    P = Placed(S, *_placement(k, nt, "one"))
    des, dts = _t(es), _t(ts)
    pos, neg = fm.split(S, es, ts)
    fits = {"matrices": FU.fit_from_matrices_dev(eng, P.ptrs, P.lds, m, nt, des.data_ptr(), dts.data_ptr(), prior),
            "lists": FU.fit_from_lists(eng, pos, neg, prior, 1e-18, 100)}
    ref = fm.fit(pos, neg, prior)
    singles = [CB.fit_from_matrix_dev(eng, P.ptrs[j], P.lds[j], m, nt, des.data_ptr(), dts.data_ptr(), prior) for j in range(k)]
    best_single = min(c.cllr_after for c in singles)
    for what, f in fits.items():
        lam2 = _assert_fit_is_optimal(f, pos, neg, k, prior)
        print("%s K %d prior %g: b = %.9g a = %s, model lambda2 there = %.3g, %d iterations, %d passes (model fit: %d, %d); "
              "Cllr %.5f, best single system %.5f" % (what, k, prior, f.b, f.a, lam2, f.iterations, f.passes, ref["iterations"],
                                                      ref["passes"], f.cllr_after, best_single))
        assert f.cllr_after <= best_single
        assert f.objective <= min(c.objective for c in singles) + 1e-12      # nested models, the same objective: guaranteed
        assert np.allclose(f.a, ref["a"], rtol=1e-6, atol=0)
    assert P.unchanged()


def test_separable_and_refused_inputs(monkeypatch):
    from plda_amd import fusion as FU
    from plda_amd._native import PLDA_E_INVAL, PldaError
    eng = _engine(monkeypatch)
    rng = np.random.default_rng(2)
    pos = [rng.uniform(5, 6, 200).astype(np.float32), rng.standard_normal(200).astype(np.float32)]
    neg = [rng.uniform(-6, -5, 3000).astype(np.float32), rng.standard_normal(3000).astype(np.float32)]
    with pytest.warns(RuntimeWarning, match="separable"):
        f = FU.fit_from_lists(eng, pos, neg)
    assert f.separable and f.cllr_after < 1e-3 and f.passes <= 100 + 30 + 2
    print("separable: a = %s, %d iterations, %d passes, converged %r" % (f.a, f.iterations, f.passes, f.converged))
    p2, n2 = [rng.standard_normal(300).astype(np.float32) + 1 for _ in range(2)], [rng.standard_normal(900).astype(np.float32) for _ in range(2)]
    bad_inf = [p2[0], p2[1].copy()]
    bad_inf[1][7] = np.inf
    cases = (([p2[0], p2[1], p2[0]], [n2[0], n2[1], n2[0]], "pivot of system 2"),
             ([p2[0], np.full(300, 1.25, np.float32)], [n2[0], np.full(900, 1.25, np.float32)], "system 1 is constant"),
             (bad_inf, n2, "1 trials with a non-finite"))
    for bp, bn, msg in cases:
        with pytest.raises(PldaError, match=msg) as ei:
            FU.fit_from_lists(eng, bp, bn)
        assert ei.value.code == PLDA_E_INVAL
    # the record of a refused pass is written all the same; a NaN in one system only counts the trial once
    bad_nan = [p2[0].copy(), p2[1].copy()]
    bad_nan[0][3] = bad_nan[1][3] = np.nan
    bad_nan[1][9] = -np.inf
    raw = np.zeros(1, FU.RECORD_DTYPE)
    pp, pn = (np.array([x.ctypes.data for x in arrs], np.uint64) for arrs in (bad_nan, n2))
    a = np.array([0.5, 0.5])
    rc = eng._lib.plda_fusion_pass_lists(eng._h, 2, C.c_void_p(pp.ctypes.data), 300, C.c_void_p(pn.ctypes.data), 900,
                                         C.c_void_p(a.ctypes.data), 0.0, 0.0, C.c_void_p(raw.ctypes.data))
    assert rc == PLDA_E_INVAL and "2 trials with a non-finite" in eng._lib.plda_last_error(eng._h).decode()
    assert int(raw["nonfinite"][0]) == 2 and int(raw["np"][0]) == 300 and int(raw["nn"][0]) == 900 and int(raw["n_systems"][0]) == 2


# ------------------------------------------------------------------------------------------- 5. the map
@pytest.mark.parametrize("m,nt,k,mode,ld_out,off_out", [(37, 500, 1, "none", 500, 0), (37, 500, 3, "one", 504, 0), (19, 1023, 8, "all", 1030, 1),
                                                       (1, 5, 3, "none", 8, 0), (33, 515, 8, "none", 516, 0)])
def test_map_is_the_fraction_chain_bit_for_bit(monkeypatch, m, nt, k, mode, ld_out, off_out):
    import torch
    from plda_amd import fusion as FU
    eng = _engine(monkeypatch)
    rng = np.random.default_rng(m + nt + k)
    S = [(rng.standard_normal((m, nt)) * 10.0 ** rng.integers(-1, 3)).astype(np.float32) for _ in range(k)]
    lds, offs = _placement(k, nt, mode)
    P = Placed(S, lds, offs)
    fus = FU.Fusion(rng.standard_normal(k) * [0.0371234567891234, 1.7, 0.3, 1.0, 2.0, 0.01, 0.5, 1.1][:k], -1.23456789012345)
    exp = fm.map_exact([s.ravel() for s in S], fus.a, fus.b).reshape(m, nt)
    G = 4096
    dO = torch.full((G + off_out + m * ld_out + G,), float(P.SENTINEL), dtype=torch.float32, device=_dev())
    FU.apply_dev(eng, P.ptrs, P.lds, m, nt, fus, dO.data_ptr() + 4 * (G + off_out), ld_out)
    eng.synchronize()
    O = dO.cpu().numpy()
    body = O[G + off_out:G + off_out + m * ld_out].reshape(m, ld_out)
    assert (O[:G + off_out] == P.SENTINEL).all() and (O[G + off_out + m * ld_out:] == P.SENTINEL).all() and (body[:, nt:] == P.SENTINEL).all()
    assert np.array_equal(exp.view(np.int32), np.ascontiguousarray(body[:, :nt]).view(np.int32))
    assert P.unchanged()
    # in place over system k - 1: the same bits, its columns beyond Nt and its guards untouched, the other systems unchanged
    j = k - 1
    FU.apply_dev(eng, P.ptrs, P.lds, m, nt, fus, P.ptrs[j], P.lds[j])
    eng.synchronize()
    flat = P.dev[j].cpu().numpy()
    inplace = flat[P.G + offs[j]:P.G + offs[j] + m * lds[j]].reshape(m, lds[j])
    assert np.array_equal(np.ascontiguousarray(inplace[:, :nt]).view(np.int32), exp.view(np.int32))
    assert (inplace[:, nt:] == P.SENTINEL).all() and (flat[:P.G + offs[j]] == P.SENTINEL).all() and (flat[P.G + offs[j] + m * lds[j]:] == P.SENTINEL).all()
    for i in range(k - 1):
        assert np.array_equal(P.dev[i].cpu().numpy().view(np.int32), P.host[i].view(np.int32))


# ------------------------------------------------------------------------------------------- 6. end to end
def test_end_to_end_plda_fuse(tmp_path):
    import torch
    from conftest import make_data
    from liblda import PLDA
    from plda_amd import fusion as FU
    x, y = make_data(61, 3000, 32, 60, scale_between=0.15)
    p = PLDA(0)
    p.fit(x, y, 5)
    enrol = p.transform(x[:180], y[:180])                                # 60 models of 3 utterances
    test = p.transform(x[1200:2400], np.arange(1200, dtype=np.uint64))   # 1200 single-utterance tests
    test_speaker = {int(i): int(s) for i, s in zip(range(1200), y[1200:2400])}
    p.norm(x[2400:], enrol)
    plain = p.score_matrix(enrol, test)
    rng = np.random.default_rng(3)
    other = (0.02 * plain.astype(np.float64) + 0.5 * rng.standard_normal(plain.shape) - 20.0).astype(np.float32)   # a second system
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                   # classes that overlap: no warning
        fus = p.fuse(enrol, test, test_speaker, [other], prior=0.5)
        fus_t = p.fuse(enrol, test, test_speaker, [_t(other)], prior=0.5)    # a torch device tensor is taken as it is
    assert fus.converged and not fus.separable and fus.n_systems == 2
    assert np.array_equal(fus.a, fus_t.a) and fus.b == fus_t.b
    assert np.array_equal(p.score_matrix(enrol, test).view(np.int32), plain.view(np.int32))        # nothing stored, defaults unchanged
    es = np.array(list(enrol.keys()), np.int64)
    ts = np.array([test_speaker[int(k)] for k in test.keys()], np.int64)
    pos, neg = fm.split([plain, other], es, ts)
    lam2 = fm.newton(fm.pass_record(pos, neg, fus.a, fus.b), 0.5)[2]
    cal = p.calibrate(enrol, test, test_speaker)
    print("end to end: a = %s, b = %.6g, Cllr fused %.4f, PLDA alone %.4f, model lambda2 = %.3g" % (fus.a, fus.b, fus.cllr_after, cal.cllr_after, lam2))
    assert lam2 <= 1e-17 and fus.cllr_after <= cal.cllr_after
    fused = p.score_matrix_fused(enrol, test, [other], fus)
    eng = p._instance
    dS, dO = _t(plain), _t(other)
    out = torch.empty_like(dS)
    torch.cuda.synchronize()
    FU.apply_dev(eng, [dS.data_ptr(), dO.data_ptr()], [1200, 1200], 60, 1200, fus, out.data_ptr(), 1200)
    eng.synchronize()
    assert np.array_equal(fused.view(np.int32), out.cpu().numpy().view(np.int32))
    sub = (slice(0, 8), slice(0, 300))
    exp = fm.map_exact([plain[sub].ravel(), other[sub].ravel()], fus.a, fus.b).reshape(8, 300)
    assert np.array_equal(np.ascontiguousarray(fused[sub]).view(np.int32), exp.view(np.int32))
    # a separable pair of systems warns as documented
    lab = es[:, None] == ts[None, :]
    sep = np.where(lab, 5.0, -5.0).astype(np.float32) + rng.uniform(-0.5, 0.5, plain.shape).astype(np.float32)
    with pytest.warns(RuntimeWarning, match="separable"):
        assert p.fuse(enrol, test, test_speaker, [sep]).separable
    # not written by save(): the file of a fused model is the file of the model
    f = str(tmp_path / "model.npz")
    p.save(f)
    assert not any("fus" in name for name in np.load(f).files)
    with pytest.raises(ValueError):
        p.fuse(enrol, test, test_speaker, [other[:, :-1]])
    with pytest.raises(ValueError):
        p.score_matrix_fused(enrol, test, [other, other], fus)


# ------------------------------------------------------------------------------------------- 7. hygiene
def _hygiene_case(rng, m, nt, k):
    es, ts = _labels(rng, m, nt, "random")
    tgt = es[:, None] == ts[None, :]
    return es, ts, _systems(rng, m, nt, k, tgt)


def test_poisoned_scratch_gives_the_same_bits(monkeypatch):
    import torch
    from plda_amd import MPlda, fusion as FU
    m, nt, k = 520, 1100, 3
    rng = np.random.default_rng(8)
    es, ts, S = _hygiene_case(rng, m, nt, k)
    pos, neg = fm.split(S, es, ts)
    a = np.array([0.2, -0.1, 0.05])
    runs = []
    for poison in (False, True):
        eng = _engine(monkeypatch, poison=poison)
        P = Placed(S, *_placement(k, nt, "one"))
        des, dts = _t(es), _t(ts)
        rec = [FU.pass_from_matrices_dev(eng, P.ptrs, P.lds, m, nt, des.data_ptr(), dts.data_ptr(), a, 0.1, 0.5),
               FU.pass_from_lists(eng, pos, neg, a, 0.1, 0.5)]
        fit = FU.fit_from_matrices_dev(eng, P.ptrs, P.lds, m, nt, des.data_ptr(), dts.data_ptr())
        out = torch.zeros((m, nt), dtype=torch.float32, device=_dev())
        torch.cuda.synchronize()
        FU.apply_dev(eng, P.ptrs, P.lds, m, nt, fit, out.data_ptr(), nt)
        eng.synchronize()
        runs.append(([{k_: np.asarray(v).tobytes() for k_, v in r.items()} for r in rec],
                     (fit.a.tobytes(), fit.b, fit.cllr_after, fit.passes), out.cpu().numpy().tobytes()))
        assert all(np.isfinite(r["L_t"]) and np.all(np.isfinite(r["H_n"])) for r in rec)
        del eng
    MPlda(0)                                   # the poison switch off again for whatever runs next in this process
    assert runs[0] == runs[1]


def test_create_fuse_destroy_gives_back_every_byte(monkeypatch):
    import gc
    import torch
    from plda_amd import _native, fusion as FU
    lib = _native.load()
    rng = np.random.default_rng(9)
    m, nt, k = 300, 400, 2
    es, ts, S = _hygiene_case(rng, m, nt, k)
    pos, neg = fm.split(S, es, ts)
    P = Placed(S, *_placement(k, nt, "none"))
    des, dts = _t(es), _t(ts)
    out = torch.zeros((m, nt), dtype=torch.float32, device=_dev())
    gc.collect()
    torch.cuda.synchronize()
    before = lib.plda_device_bytes_held()
    for _ in range(3):
        eng = _engine(monkeypatch)
        f = FU.fit_from_matrices_dev(eng, P.ptrs, P.lds, m, nt, des.data_ptr(), dts.data_ptr())
        assert lib.plda_device_bytes_held() > before
        FU.fit_from_lists(eng, pos, neg, 0.1)
        FU.apply_dev(eng, P.ptrs, P.lds, m, nt, f, out.data_ptr(), nt)
        eng.synchronize()
        del eng
        gc.collect()
        assert lib.plda_device_bytes_held() == before


def test_api_edges(monkeypatch):
    from plda_amd import fusion as FU
    from plda_amd._native import PLDA_E_INVAL
    eng = _engine(monkeypatch)
    lib, h = eng._lib, eng._h
    rng = np.random.default_rng(10)
    m, nt, k = 20, 30, 2
    es, ts, S = _hygiene_case(rng, m, nt, k)
    dS = [_t(s) for s in S]
    des, dts, dO = _t(es), _t(ts), _t(np.zeros((m, nt), np.float32))
    rec, fit = np.zeros(1, FU.RECORD_DTYPE), np.zeros(1, FU.FIT_DTYPE)
    vp = lambda arr: C.c_void_p(arr.ctypes.data)                                    # noqa: E731
    tp = lambda t: C.c_void_p(t.data_ptr())                                         # noqa: E731
    R, F = vp(rec), vp(fit)
    ptrs = np.array([d.data_ptr() for d in dS] + [0] * 7, np.uint64)
    null1 = ptrs.copy()
    null1[1] = 0
    ld = np.full(9, nt, np.int64)
    ld_short = ld.copy()
    ld_short[1] = nt - 1
    a = np.zeros(9)
    pos, neg = fm.split(S, es, ts)
    np_, nn_ = pos[0].shape[0], neg[0].shape[0]
    pp = np.array([x.ctypes.data for x in pos] + [0] * 7, np.uint64)
    pn = np.array([x.ctypes.data for x in neg] + [0] * 7, np.uint64)
    pmat = lambda K=k, P=ptrs, L=ld, M=m, Nt=nt, E=tp(des), T=tp(dts), A=vp(a), O=R: lib.plda_fusion_pass_matrices_dev(  # noqa: E731
        h, K, vp(P) if P is not None else None, vp(L) if L is not None else None, M, Nt, E, T, A, 0.0, 0.0, O)
    fmat = lambda K=k, P=ptrs, L=ld, M=m, Nt=nt, prior=0.5, tol=0.0, O=F: lib.plda_fusion_fit_matrices_dev(  # noqa: E731
        h, K, vp(P), vp(L), M, Nt, tp(des), tp(dts), prior, tol, 0, O)
    mapd = lambda K=k, P=ptrs, L=ld, M=m, Nt=nt, A=vp(a), O=tp(dO), ldo=nt: lib.plda_fusion_map_dev(h, K, vp(P), vp(L), M, Nt, A, 0.0, O, ldo)  # noqa: E731
    bad = [
        pmat(K=0), pmat(K=9), pmat(K=-1), pmat(P=null1), pmat(P=None), pmat(L=None), pmat(L=ld_short), pmat(M=0), pmat(Nt=0), pmat(M=-3),
        pmat(E=None), pmat(T=None), pmat(A=None), pmat(O=None),
        fmat(K=0), fmat(K=9), fmat(P=null1), fmat(L=ld_short), fmat(M=0), fmat(Nt=-1), fmat(prior=0.0), fmat(prior=1.0),
        fmat(prior=float("nan")), fmat(prior=-0.1), fmat(tol=-1.0), fmat(O=None),
        mapd(K=0), mapd(K=9), mapd(P=null1), mapd(L=ld_short), mapd(M=0), mapd(Nt=0), mapd(A=None), mapd(O=None), mapd(ldo=nt - 1),
        lib.plda_fusion_pass_lists(h, 0, vp(pp), np_, vp(pn), nn_, vp(a), 0.0, 0.0, R),
        lib.plda_fusion_pass_lists(h, 9, vp(pp), np_, vp(pn), nn_, vp(a), 0.0, 0.0, R),
        lib.plda_fusion_pass_lists(h, 3, vp(pp), np_, vp(pn), nn_, vp(a), 0.0, 0.0, R),          # the third list is NULL
        lib.plda_fusion_pass_lists(h, k, None, np_, vp(pn), nn_, vp(a), 0.0, 0.0, R),
        lib.plda_fusion_pass_lists(h, k, vp(pp), 0, vp(pn), nn_, vp(a), 0.0, 0.0, R),
        lib.plda_fusion_pass_lists(h, k, vp(pp), np_, vp(pn), nn_, None, 0.0, 0.0, R),
        lib.plda_fusion_pass_lists(h, k, vp(pp), np_, vp(pn), nn_, vp(a), 0.0, 0.0, None),
        lib.plda_fusion_fit_lists(h, k, vp(pp), np_, vp(pn), 0, 0.5, 0.0, 0, F),
        lib.plda_fusion_fit_lists(h, k, vp(pp), np_, vp(pn), nn_, 1.5, 0.0, 0, F),
        lib.plda_fusion_fit_lists(h, k, vp(pp), np_, vp(pn), nn_, 0.5, -1.0, 0, F),
        lib.plda_fusion_fit_lists(h, k, vp(pp), np_, vp(pn), nn_, 0.5, 0.0, 0, None),
        lib.plda_fusion_pass_matrices_dev(None, k, vp(ptrs), vp(ld), m, nt, tp(des), tp(dts), vp(a), 0.0, 0.0, R),
        lib.plda_fusion_newton(None, 0.5, None, None, None),
    ]
    assert bad == [PLDA_E_INVAL] * len(bad), bad
    assert pmat(L=ld_short) == PLDA_E_INVAL and "ld[1]" in lib.plda_last_error(h).decode()
    assert pmat(P=null1) == PLDA_E_INVAL and "system 1 is NULL" in lib.plda_last_error(h).decode()
    # one class only: every trial a target
    one = _t(np.zeros(m, np.int64)), _t(np.zeros(nt, np.int64))
    assert pmat(E=tp(one[0]), T=tp(one[1])) == PLDA_E_INVAL
    assert "at least one target" in lib.plda_last_error(h).decode()
    assert int(rec["np"][0]) == m * nt and int(rec["nn"][0]) == 0 and int(rec["n_systems"][0]) == k      # written all the same
    # and the handle still works
    w = np.array([0.3, -0.2])
    theta = _theta(S, w, 0.1)
    got = FU.pass_from_matrices_dev(eng, [d.data_ptr() for d in dS], [nt, nt], m, nt, des.data_ptr(), dts.data_ptr(), w, 0.1, theta)
    _compare("after the edges", got, fm.pass_matrices(S, es, ts, w, 0.1, theta))
    eng.synchronize()
    assert np.array_equal(dO.cpu().numpy(), np.zeros((m, nt), np.float32))   # no refused map wrote anything
