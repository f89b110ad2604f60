"""GPU: linear score calibration, Cllr and actual DCF (csrc/calib.hip; include/plda_hip.h "linear score calibration"),
every call through the C ABI, against the host model tests/calibration_model.py.

  1. the pass record against the model over the loaders' shapes and four (a, c) points: integers, min and max exactly, each
     sum within 1e-12 * sum|term| (derived in the header: per-term error < 8.4e-14, a tree sum adds 34 u; a factor of ten left);
  2. determinism: the same call twice is bit-identical (the grid is a function of the shape, not tunable);
  3. matrix, list and operand forms agree; the operand form sees the scores of plda_score_matrix_dev bit for bit;
  4. the fit: optimality at the returned point by the MODEL's gradient and Hessian, Cllr after, equivariance, the Gaussian
     closed form, the pass count;
  5. plda_affine_map_dev: the correctly rounded fp32 of fma(a, s, b), in place, guard columns untouched;
  6. liblda.PLDA end to end (z-norm and AS-norm), actDCF, save / load;
  7. 20 000 x 50 000 against the chunked host model, 100 000 x 100 000 matrix form against operand form, slab cap asserted;
  8. guard bands, poisoned scratch, create / calibrate / destroy, API edges.

Run with -s to see the measured figures next to each bound.  Nothing here provokes a fault."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import calibration_model as cm
from test_calibration_model import gaussian_case, gaussian_standard_errors

pytestmark = pytest.mark.gpu

ENV = ("PLDA_EER_SLAB_ROWS", "PLDA_SCRATCH_POISON", "PLDA_EER_VARIANT")
BOUND = 1e-12
INTS = ("Np", "Nn", "miss", "fa", "nonfinite", "min_t", "max_t", "min_n", "max_n")
SUMS = [n + c for c in ("_t", "_n") for n in cm.SUMS]


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _engine(monkeypatch, d=32, slab=None, poison=False):
    from plda_amd import MPlda
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    if slab:
        monkeypatch.setenv("PLDA_EER_SLAB_ROWS", str(slab))
    if poison:
        monkeypatch.setenv("PLDA_SCRATCH_POISON", "1")
    eng = MPlda(0)
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    rng = np.random.default_rng(d)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    eng.set_model(rng.random(d), q * (1.0 + rng.random(d))[:, None], np.sort(0.05 + rng.random(d) * 4.0)[::-1].copy())
    return eng


def _labels(rng, m, nt, k):
    es, ts = rng.integers(0, k, m), rng.integers(0, k, nt)
    es[0] = ts[0] = 0                       # at least one target ...
    if nt > 1:
        ts[-1] = k                          # ... and one non-target (a speaker nobody enrolled)
    else:
        es[-1] = k
    return es.astype(np.int64), ts.astype(np.int64)


def _compare(what, got, ref, scale=None):
    """Integers and extremes exactly; each sum within BOUND * sum|term| (the model's `abs`, or `scale`)."""
    for k in INTS:
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    worst = 0.0
    for k in SUMS:
        s = (scale or ref["abs"])[k]
        err = abs(got[k] - ref[k])
        if s == 0.0:
            assert err == 0.0, (what, k, got[k], ref[k])
            continue
        worst = max(worst, err / s)
        assert err <= BOUND * s, (what, k, got[k], ref[k], err / s)
    print("%s: max |sum - model| / sum|term| = %.3g (bound %.0e)" % (what, worst, BOUND))


def _points(pos, neg):
    """(a, c): the start, the identity, a fitted point, a saturating point (|y| of a few hundred)."""
    f = cm.fit(pos[:4000], neg[:40000])
    smax = float(max(np.abs(pos).max(), np.abs(neg).max()))
    return [(0.0, 0.0), (1.0, 0.0), (f["a"], f["b"]), (300.0 / smax, 5.0)]


# ------------------------------------------------------------------------------------------- 1. + 2. the pass record
@pytest.mark.parametrize("m,nt,ld,off,k", [(300, 500, 500, 0, 12), (300, 500, 512, 0, 12), (37, 1023, 1023, 0, 5), (64, 512, 512, 1, 6),
                                           (1, 2000, 2000, 0, 3), (700, 1, 1, 0, 4), (5, 4099, 4100, 0, 5), (4096, 8192, 8192, 0, 200),
                                           (513, 1025, 1028, 1, 16)])
def test_pass_record_matches_the_model(monkeypatch, m, nt, ld, off, k):
    """ld > Nt, Nt not a multiple of 4, a misaligned base pointer (off: floats), one row, one column, 300 x 500, 4096 x 8192;
    513 x 1025 under ld = 1028 from a base pointer one float off: a second column strip of one column."""
    from plda_amd import calibration as CB
    eng = _engine(monkeypatch)
    rng = np.random.default_rng(m * 7919 + nt + ld)
    es, ts = _labels(rng, m, nt, k)
    tgt = es[:, None] == ts[None, :]
    Sh = (rng.standard_normal((m, ld)) * 3.0).astype(np.float32)
    Sh[:, :nt] += np.float32(4.0) * tgt
    flat = np.concatenate([np.zeros(off, np.float32), Sh.ravel()])
    dS, des, dts = _t(flat), _t(es), _t(ts)
    ptr = dS.data_ptr() + 4 * off
    sub = Sh[:, :nt]
    pos, neg = sub[tgt], sub[~tgt]
    for a, c in _points(pos, neg):
        theta = 0.7
        got = CB.pass_from_matrix_dev(eng, ptr, ld, m, nt, des.data_ptr(), dts.data_ptr(), a, c, theta)
        again = CB.pass_from_matrix_dev(eng, ptr, ld, m, nt, des.data_ptr(), dts.data_ptr(), a, c, theta)
        for key in got:                                        # 2. determinism: bit-identical
            assert np.asarray(got[key]).tobytes() == np.asarray(again[key]).tobytes(), key
        ref = cm.pass_matrix(sub, es, ts, a, c, theta)
        _compare("%dx%d ld %d off %d at (%.3g, %.3g)" % (m, nt, ld, off, a, c), got, ref)
        assert got["Np"] == int(tgt.sum()) and got["Np"] + got["Nn"] == m * nt


def test_list_form_matches_the_model_and_is_deterministic(monkeypatch):
    from plda_amd import calibration as CB
    eng = _engine(monkeypatch)
    rng = np.random.default_rng(4)
    for npos, nneg in ((1, 1), (3, 70000), (2_000_003, 5), (1, 70000), (70000, 1)):
        pos = (2.0 + rng.standard_normal(npos) * 2).astype(np.float32)
        neg = (-2.0 + rng.standard_normal(nneg) * 2).astype(np.float32)
        for a, c in ((0.0, 0.3), (1.0, 0.0), (60.0, -3.0)):
            got = CB.pass_from_lists(eng, pos, neg, a, c, -0.25)
            assert got == CB.pass_from_lists(eng, pos, neg, a, c, -0.25)
            _compare("lists %d + %d at (%g, %g)" % (npos, nneg, a, c), got, cm.pass_record(pos, neg, a, c, -0.25))


# ------------------------------------------------------------------------------------------- 3. three sources, one answer
def _operands(rng, m, nt, d, mixed):
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    n = rng.integers(1, 4, m).astype(np.int32) if mixed else 2
    return U, V, n


def _score_matrix(eng, dU, dn, nu, m, dV, nt, dzm=None, dzs=None):
    import torch
    S = torch.empty((m, nt), dtype=torch.float32, device=_dev())
    eng.score_matrix_dev(dU.data_ptr(), dn.data_ptr() if dn is not None else None, nu, m, dV.data_ptr(), nt, S.data_ptr(), nt,
                         dzm.data_ptr() if dzm is not None else None, dzs.data_ptr() if dzs is not None else None)
    eng.synchronize()
    return S


@pytest.mark.parametrize("mixed,zn,m,nt", [(False, False, 900, 1300), (True, True, 900, 1300), (True, True, 513, 1025)],
                         ids=["False-False", "True-True", "True-True-513x1025"])
def test_three_sources_one_answer(monkeypatch, mixed, zn, m, nt):
    from plda_amd import calibration as CB
    d = 48
    eng = _engine(monkeypatch, d, slab=256)                    # 900 rows: four slabs; 513 rows: three, the last of one row
    rng = np.random.default_rng(31 + mixed)
    U, V, n = _operands(rng, m, nt, d, mixed)
    es, ts = _labels(rng, m, nt, 30)
    dU, dV, des, dts = _t(U), _t(V), _t(es), _t(ts)
    dn = _t(n) if mixed else None
    nu = 0 if mixed else int(n)
    dzm, dzs = (_t(rng.standard_normal(m)), _t(0.5 + rng.random(m))) if zn else (None, None)
    S = _score_matrix(eng, dU, dn, nu, m, dV, nt, dzm, dzs)
    Sh = S.cpu().numpy()
    pos, neg = cm.split(Sh, es, ts)
    f = cm.fit(pos, neg)
    for a, c, theta in ((1.0, 0.0, 0.0), (f["a"], f["b"], -f["b"] / f["a"])):
        ref = cm.pass_matrix(Sh, es, ts, a, c, theta)
        mat = CB.pass_from_matrix_dev(eng, S.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr(), a, c, theta)
        lst = CB.pass_from_lists(eng, pos, neg, a, c, theta)
        opr = CB.pass_from_operands_dev(eng, dU.data_ptr(), dn.data_ptr() if mixed else None, nu, m, dV.data_ptr(), nt,
                                        des.data_ptr(), dts.data_ptr(), dzm.data_ptr() if zn else None, dzs.data_ptr() if zn else None,
                                        a, c, theta)
        for what, got in (("matrix", mat), ("lists", lst), ("operands, slabs of 256 rows", opr)):
            _compare("%s at (%.3g, %.3g)" % (what, a, c), got, ref)
        # bit for bit the same scores: the extremes and every exact count already agree; the sums of the operand form
        # are those of the matrix form over the same values in another order


# ------------------------------------------------------------------------------------------- 4. the fit
def _optimality(pos, neg, a, b, prior):
    rec = cm.pass_record(pos, neg, a, b + cm.logit(prior))
    return cm.solve2(cm.hessian(rec, prior), cm.gradient(rec, prior))[1]


def _assert_fit_is_optimal(what, f, pos, neg, prior, tol, ref=None):
    """the optimality rule: the MODEL's own lambda2 at the device's (a, b) is at most 10 * tol; Cllr before and after within
    BOUND of the model's; the pass count"""
    lam2 = _optimality(pos, neg, f.a, f.b, prior)
    print("%s prior %g: a = %.12g b = %.12g, model lambda2 there = %.3g (tol %g), %d iterations, %d passes%s"
          % (what, prior, f.a, f.b, lam2, tol, f.iterations, f.passes, "; model fit: %d, %d" % (ref["iterations"], ref["passes"]) if ref else ""))
    assert f.converged and not f.separable
    assert lam2 <= 10 * tol
    after = cm.pass_record(pos, neg, f.a, f.b)
    scale = 0.5 / after["Np"] * after["abs"]["L_t"] + 0.5 / after["Nn"] * after["abs"]["L_n"]
    assert abs(f.cllr_after * cm.LN2 - cm.objective(after, 0.5)) <= BOUND * scale
    before = cm.pass_record(pos, neg, 1.0, 0.0)
    scale = 0.5 / before["Np"] * before["abs"]["L_t"] + 0.5 / before["Nn"] * before["abs"]["L_n"]
    assert abs(f.cllr_before * cm.LN2 - cm.objective(before, 0.5)) <= BOUND * scale
    assert f.cllr_after <= min(1.0, f.cllr_before)
    assert 0 < f.passes <= 100 + 30 and f.prior == prior


def _assert_equivariant(f, f2, k, d):
    """f2 is the fit of the scores k * s + d: the map undoes the scale and the shift"""
    assert cm.equivariant(f.a, f.b, f2.a, f2.b, k, d), (f.a, f.b, f2.a, f2.b, k, d)


@pytest.mark.parametrize("prior", [0.5, 0.05])
def test_fit_is_optimal_by_the_models_own_derivatives(monkeypatch, prior):
    from plda_amd import calibration as CB
    eng = _engine(monkeypatch)
    rng = np.random.default_rng(41)
    m, nt = 700, 1900
    es, ts = _labels(rng, m, nt, 25)
    tgt = es[:, None] == ts[None, :]
    Sh = (rng.standard_normal((m, nt)) * 6.0 + 9.0 * tgt - 20.0).astype(np.float32)
    pos, neg = Sh[tgt], Sh[~tgt]
    dS, des, dts = _t(Sh), _t(es), _t(ts)
    tol = 1e-18
    fits = {"matrix": CB.fit_from_matrix_dev(eng, dS.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr(), prior),
            "lists": CB.fit_from_lists(eng, pos, neg, prior, tol, 100)}
    ref = cm.fit(pos, neg, prior)
    for what, f in fits.items():
        _assert_fit_is_optimal(what, f, pos, neg, prior, tol, ref)


def test_fit_off_prior_half_on_a_lopsided_set(monkeypatch):
    """Found by the sweep (tests/test_gpu_sweep.py, PLDA_SWEEP_SEED=1, calibration-10): 254 targets on six score values against
    ONE non-target in their midst, prior 0.05.  The device's fit is the optimum of the prior-weighted objective (the model's
    lambda2 there is within the rule) and its Cllr figures are the model's -- but Cllr after, which is taken at prior 0.5, is
    1.07: `cllr_after <= min(1, cllr_before)` is a law only where the fit minimises Cllr itself, at prior 0.5."""
    from plda_amd import calibration as CB
    eng = _engine(monkeypatch)
    pos = np.repeat(np.float32([-1, 0, 1, 2, 3, 4]), [3, 19, 66, 95, 54, 17])
    neg = np.float32([2.0])
    tol = 1e-18
    f = CB.fit_from_lists(eng, pos, neg, 0.05, tol, 100)
    ref = cm.fit(pos, neg, 0.05)
    assert f.converged and not f.separable and _optimality(pos, neg, f.a, f.b, 0.05) <= 10 * tol
    after = cm.pass_record(pos, neg, f.a, f.b)
    scale = 0.5 / after["Np"] * after["abs"]["L_t"] + 0.5 / after["Nn"] * after["abs"]["L_n"]
    assert abs(f.cllr_after * cm.LN2 - cm.objective(after, 0.5)) <= BOUND * scale
    print("prior 0.05: a = %.12g b = %.12g, Cllr %.6f -> %.6f (model %.6f)" % (f.a, f.b, f.cllr_before, f.cllr_after, ref["cllr_after"]))
    assert f.a < 0 and 1.0 < f.cllr_after < f.cllr_before and ref["cllr_after"] > 1.0
    _assert_fit_is_optimal("prior 0.5", CB.fit_from_lists(eng, pos, neg, 0.5, tol, 100), pos, neg, 0.5, tol)      # the whole rule holds there


def test_fit_equivariance_and_gaussian_closed_form(monkeypatch):
    from plda_amd import calibration as CB
    eng = _engine(monkeypatch)
    pos, neg, a_true = gaussian_case()
    f = CB.fit_from_lists(eng, pos, neg)
    se_a, se_b = gaussian_standard_errors(pos, neg, f.a, f.b)
    print("Gaussian: a = %.6f (true %.3f, se %.4f), b = %.6f (se %.4f)" % (f.a, a_true, se_a, f.b, se_b))
    assert abs(f.a - a_true) <= 5 * se_a and abs(f.b) <= 5 * se_b
    k, d = 8.0, -3.0
    f2 = CB.fit_from_lists(eng, (k * pos.astype(np.float64) + d).astype(np.float32), (k * neg.astype(np.float64) + d).astype(np.float32))
    _assert_equivariant(f, f2, k, d)
    f3 = CB.fit_from_lists(eng, f(pos).astype(np.float32), f(neg).astype(np.float32))
    assert f3.a == pytest.approx(1.0, abs=1e-5) and f3.b == pytest.approx(0.0, abs=1e-5)


def test_separable_and_degenerate_inputs(monkeypatch):
    from plda_amd import calibration as CB
    from plda_amd._native import PLDA_E_INVAL, PldaError
    eng = _engine(monkeypatch)
    rng = np.random.default_rng(2)
    pos, neg = rng.uniform(5, 6, 200).astype(np.float32), rng.uniform(-6, -5, 3000).astype(np.float32)
    with pytest.warns(RuntimeWarning, match="separable"):
        f = CB.fit_from_lists(eng, pos, neg)
    assert f.separable and f.cllr_after < 1e-3 and f.passes <= 100 + 30 + 2
    print("separable: a = %g, %d iterations, %d passes, converged %r" % (f.a, f.iterations, f.passes, f.converged))
    same = np.full(50, 1.25, np.float32)
    for bad_pos, bad_neg, msg in ((same, same, "equal"), (np.float32([1.0, np.inf]), np.float32([0.0, -1.0]), "1 non-finite"),
                                  (np.float32([1.0, np.nan, np.nan]), np.float32([0.0]), "2 non-finite")):
        with pytest.raises(PldaError, match=msg) as ei:
            CB.fit_from_lists(eng, bad_pos, bad_neg)
        assert ei.value.code == PLDA_E_INVAL


# ------------------------------------------------------------------------------------------- 5. apply
def _expected_map(s32, a, b, got):
    """The correctly rounded fp32 of fl64(a * s + b): np.longdouble first, and where that and the device differ by one
    fp32 ulp the case is decided exactly with fractions.Fraction."""
    exp = cm.apply_map(s32, a, b)
    diff = np.nonzero(exp.view(np.int32) != got.view(np.int32))[0]
    for i in diff:
        exact = Fraction(float(a)) * Fraction(float(s32[i])) + Fraction(float(b))
        exp[i] = np.float32(float(exact))                     # Fraction -> float and float -> float32 both round correctly
    return exp, diff.size


@pytest.mark.parametrize("m,nt,ld,ld_out,off", [(300, 500, 500, 500, 0), (37, 1023, 1024, 1030, 0), (64, 512, 512, 512, 1), (1, 5, 5, 8, 0),
                                                (2100, 4096, 4096, 4096, 0)])
def test_affine_map_rounding_in_place_and_guards(monkeypatch, m, nt, ld, ld_out, off):
    import torch
    from plda_amd import calibration as CB
    eng = _engine(monkeypatch)
    rng = np.random.default_rng(m + nt)
    cal = CB.Calibration(0.0371234567891234, -1.23456789012345)
    Sh = (rng.standard_normal((m, ld)) * 40).astype(np.float32)
    dS = _t(np.concatenate([np.zeros(off, np.float32), Sh.ravel()]))
    sentinel = np.float32(-7.25e30)
    G = 4096                                                            # guard floats before and after the output
    dO = torch.full((G + off + m * ld_out + G,), float(sentinel), dtype=torch.float32, device=_dev())
    CB.apply_dev(eng, dS.data_ptr() + 4 * off, ld, m, nt, cal, dO.data_ptr() + 4 * (G + off), ld_out)
    eng.synchronize()
    O = dO.cpu().numpy()
    body = O[G + off:G + off + m * ld_out].reshape(m, ld_out)
    assert (O[:G + off] == sentinel).all() and (O[G + off + m * ld_out:] == sentinel).all() and (body[:, nt:] == sentinel).all()
    exp, decided = _expected_map(Sh[:, :nt].ravel(), cal.a, cal.b, body[:, :nt].ravel().copy())
    assert np.array_equal(exp.view(np.int32), body[:, :nt].ravel().view(np.int32))
    print("affine map %dx%d: %d elements decided by exact arithmetic" % (m, nt, decided))
    # in place: same bits, and the columns beyond Nt keep their scores
    CB.apply_dev(eng, dS.data_ptr() + 4 * off, ld, m, nt, cal)
    eng.synchronize()
    inplace = dS.cpu().numpy()[off:].reshape(m, ld)
    assert np.array_equal(inplace[:, :nt].view(np.int32), body[:, :nt].view(np.int32))
    assert np.array_equal(inplace[:, nt:].view(np.int32), Sh[:, nt:].view(np.int32))


# ------------------------------------------------------------------------------------------- 6. end to end
def test_end_to_end_plda_calibrate(tmp_path):
    from conftest import make_data
    from liblda import PLDA
    from plda_amd import calibration as CB
    x, y = make_data(61, 3000, 32, 60, scale_between=0.15)               # real speaker structure, classes that overlap
    p = PLDA(0)
    p.fit(x, y, 5)
    enrol = p.transform(x[:180], y[:180])                                # 60 models of 3 utterances
    test = p.transform(x[1200:2400], np.arange(1200, dtype=np.uint64))   # 1200 single-utterance tests
    test_speaker = {int(i): int(s) for i, s in zip(range(1200), y[1200:2400])}
    p.norm(x[2400:], enrol)                                              # 600 held-out rows: z-norm background, AS-norm cohort
    with pytest.raises(ValueError, match="stored calibration"):
        p.score_matrix(enrol, test, calibrate=True)
    plain = p.score_matrix(enrol, test)
    cal = p.calibrate(enrol, test, test_speaker, prior=0.5)
    assert cal.converged and not cal.separable and cal.cllr_after <= min(1.0, cal.cllr_before)
    assert np.array_equal(p.score_matrix(enrol, test).view(np.int32), plain.view(np.int32))        # defaults unchanged
    mapped = p.score_matrix(enrol, test, calibrate=True)
    exp, _ = _expected_map(plain.ravel(), cal.a, cal.b, mapped.ravel().copy())
    assert np.array_equal(exp.view(np.int32), mapped.ravel().view(np.int32))
    # the fit is the model's optimum on the matrix the library scores
    es = np.array(list(enrol.keys()), np.int64)
    ts = np.array([test_speaker[int(k)] for k in test.keys()], np.int64)
    pos, neg = cm.split(plain, es, ts)
    lam2 = _optimality(pos, neg, cal.a, cal.b, 0.5)
    print("end to end: a = %.6g, b = %.6g, Cllr %.4f -> %.4f, model lambda2 = %.3g" % (cal.a, cal.b, cal.cllr_before, cal.cllr_after, lam2))
    assert lam2 <= 1e-17
    # actDCF of the calibrated matrix at pi = 0.5 equals the host count
    cpos, cneg = cm.split(mapped, es, ts)
    eng = p._instance
    dcf = CB.act_dcf(lambda th: CB.pass_from_lists(eng, cpos, cneg, 1.0, 0.0, th), 0.5)
    assert dcf == cm.act_dcf(cpos, cneg, 0.5)
    assert dcf == ((cpos.astype(np.float64) < 0.0).mean() + (cneg.astype(np.float64) >= 0.0).mean())
    # trial lists: a * s + b in fp64
    e_idx, t_idx = np.array([0, 5, 59]), np.array([7, 0, 1199])
    assert np.array_equal(p.score_trials(enrol, test, e_idx, t_idx, calibrate=True), cal(p.score_trials(enrol, test, e_idx, t_idx)))
    # save / load round trip; a file without the keys clears the calibration
    f = str(tmp_path / "model.npz")
    p.save(f)
    q = PLDA(0)
    q.load(f)
    c2 = q._instance.calibration
    assert (c2.a, c2.b, c2.prior) == (cal.a, cal.b, cal.prior)
    assert np.array_equal(q.score_matrix(enrol, test, calibrate=True).view(np.int32), mapped.view(np.int32))
    r = PLDA(0)
    r.fit(x, y, 5)
    g = str(tmp_path / "plain.npz")
    r.save(g)                                                             # written through the unchanged path
    assert "calib_a" not in np.load(g).files
    q.load(g)
    assert q._instance.calibration is None
    with pytest.raises(ValueError):
        q.score_matrix(enrol, test, calibrate=True)
    # AS-norm variant
    cohort = p.transform_array(x[2400:], 1)
    raw_as = p.score_matrix_asnorm(enrol, test, cohort, top_k=100)
    cal_as = p.calibrate(enrol, test, test_speaker, cohort=cohort, top_k=100)
    assert np.array_equal(p.score_matrix_asnorm(enrol, test, cohort, top_k=100).view(np.int32), raw_as.view(np.int32))
    mapped_as = p.score_matrix_asnorm(enrol, test, cohort, top_k=100, calibrate=True)
    exp, _ = _expected_map(raw_as.ravel(), cal_as.a, cal_as.b, mapped_as.ravel().copy())
    assert np.array_equal(exp.view(np.int32), mapped_as.ravel().view(np.int32))
    pos, neg = cm.split(raw_as, es, ts)
    assert _optimality(pos, neg, cal_as.a, cal_as.b, 0.5) <= 1e-17
    tr = p.score_trials_asnorm(enrol, test, e_idx, t_idx, cohort, top_k=100)
    assert np.array_equal(p.score_trials_asnorm(enrol, test, e_idx, t_idx, cohort, top_k=100, calibrate=True), cal_as(tr))


# ------------------------------------------------------------------------------------------- 7. scale
def test_scale_1e9_against_the_chunked_model(monkeypatch):
    """20 000 x 50 000 = 1e9 trials, 20 utterances per speaker on the test side (a 1e-3 share of targets)."""
    import torch
    from plda_amd import calibration as CB
    eng = _engine(monkeypatch)
    dev = _dev()
    m, nt = 20000, 50000
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    es, ts = torch.arange(m, device=dev) // 20, torch.arange(nt, device=dev) // 50
    S = torch.randn((m, nt), dtype=torch.float32, device=dev, generator=g) * 5.0 - 8.0
    for r0 in range(0, m, 4000):
        S[r0:r0 + 4000] += 12.0 * (es[r0:r0 + 4000, None] == ts[None, :])
    a, c, theta = 0.31, 1.9, -4.0
    torch.cuda.synchronize()                                             # (the engine runs on its own stream)
    got = CB.pass_from_matrix_dev(eng, S.data_ptr(), nt, m, nt, es.data_ptr(), ts.data_ptr(), a, c, theta)
    esh, tsh = es.cpu().numpy(), ts.cpu().numpy()
    acc = cm.Acc(fast=True)
    for r0 in range(0, m, 400):
        pos, neg = cm.split(S[r0:r0 + 400].cpu().numpy(), esh[r0:r0 + 400], tsh)
        acc.add(pos, a, c, theta, True)
        acc.add(neg, a, c, theta, False)
    _compare("20000 x 50000", got, acc.record())


def test_scale_1e10_matrix_form_against_operand_form(monkeypatch):
    """100 000 x 100 000: the host model is not run on 1e10 trials; the matrix form (40 GB of scores held) is compared with the
    operand form, which holds one slab beyond the packed operands (asserted through plda_device_bytes_peak).  The band uses
    |sum| in place of sum|term| (never larger: a narrower band than item 1's)."""
    import torch
    from plda_amd import _native, calibration as CB
    lib = _native.load()
    dev = _dev()
    d, m, nt = 64, 100000, 100000
    eng = _engine(monkeypatch, d)
    g = torch.Generator(device=dev)
    g.manual_seed(6)
    U = torch.randn((m, d), dtype=torch.float64, device=dev, generator=g)
    V = torch.randn((nt, d), dtype=torch.float64, device=dev, generator=g)
    es, ts = torch.arange(m, device=dev) // 20, torch.arange(nt, device=dev) // 20
    a, c, theta = 0.05, -0.4, 3.0
    torch.cuda.synchronize()
    before = lib.plda_device_bytes_held()
    lib.plda_device_bytes_peak(1)
    opr = CB.pass_from_operands_dev(eng, U.data_ptr(), None, 2, m, V.data_ptr(), nt, es.data_ptr(), ts.data_ptr(), None, None, a, c, theta)
    rose = lib.plda_device_bytes_peak(0) - before
    pad = lambda v, q: (v + q - 1) // q * q                                         # noqa: E731
    kpad = pad(d + 1, 4) + 32
    slab_rows = pad(min(m, (4 << 30) // 4 // nt), 256)
    operands = (slab_rows + pad(nt, 256)) * kpad * 4 + (slab_rows + pad(nt, 256)) * 4 * 8
    operands += operands // 8 + (8 << 20)
    slab = slab_rows * nt * 4
    print("1e10 operand form: device bytes rose by %.1f MiB (one slab of %.1f MiB + %.1f MiB allowed for packed operands and partial records)"
          % (rose / 2 ** 20, slab / 2 ** 20, operands / 2 ** 20))
    assert rose <= slab + slab // 8 + operands
    S = _score_matrix(eng, U, None, 2, m, V, nt)
    mat = CB.pass_from_matrix_dev(eng, S.data_ptr(), nt, m, nt, es.data_ptr(), ts.data_ptr(), a, c, theta)
    assert mat["Np"] == 20 * m and mat["Np"] + mat["Nn"] == m * nt
    _compare("1e10 matrix vs operands", mat, opr, scale={k: abs(opr[k]) for k in SUMS})


# ------------------------------------------------------------------------------------------- 8. hygiene
def test_poisoned_scratch_gives_the_same_bits(monkeypatch):
    from plda_amd import MPlda, calibration as CB
    d, m, nt = 40, 520, 777
    rng = np.random.default_rng(8)
    U, V, n = _operands(rng, m, nt, d, True)
    es, ts = _labels(rng, m, nt, 20)
    runs = []
    for poison in (False, True):
        eng = _engine(monkeypatch, d, slab=256, poison=poison)
        dU, dV, dn, des, dts = _t(U), _t(V), _t(n), _t(es), _t(ts)
        S = _score_matrix(eng, dU, dn, 0, m, dV, nt)
        Sh = S.cpu().numpy()
        pos, neg = cm.split(Sh, es, ts)
        rec = [CB.pass_from_matrix_dev(eng, S.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr(), 0.2, 0.1, 0.5),
               CB.pass_from_operands_dev(eng, dU.data_ptr(), dn.data_ptr(), 0, m, dV.data_ptr(), nt, des.data_ptr(), dts.data_ptr(),
                                         None, None, 0.2, 0.1, 0.5),
               CB.pass_from_lists(eng, pos, neg, 0.2, 0.1, 0.5)]
        fit = CB.fit_from_operands_dev(eng, dU.data_ptr(), dn.data_ptr(), 0, m, dV.data_ptr(), nt, des.data_ptr(), dts.data_ptr())
        runs.append((rec, (fit.a, fit.b, fit.cllr_after, fit.passes)))
        del eng
    MPlda(0)                                   # the poison switch off again for whatever runs next in this process
    assert runs[0] == runs[1]
    assert all(np.isfinite(r[k]) for r in runs[1][0] for k in SUMS)


def test_create_calibrate_destroy_gives_back_every_byte(monkeypatch):
    import gc
    import torch
    from plda_amd import _native, calibration as CB
    lib = _native.load()
    rng = np.random.default_rng(9)
    d, m, nt = 32, 300, 400
    U, V, _ = _operands(rng, m, nt, d, False)
    es, ts = _labels(rng, m, nt, 10)
    dU, dV, des, dts = _t(U), _t(V), _t(es), _t(ts)
    gc.collect()
    torch.cuda.synchronize()
    before = lib.plda_device_bytes_held()
    for _ in range(3):
        eng = _engine(monkeypatch, d)
        S = _score_matrix(eng, dU, None, 1, m, dV, nt)
        f = CB.fit_from_matrix_dev(eng, S.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr())
        CB.fit_from_operands_dev(eng, dU.data_ptr(), None, 1, m, dV.data_ptr(), nt, des.data_ptr(), dts.data_ptr())
        CB.apply_dev(eng, S.data_ptr(), nt, m, nt, f)
        assert lib.plda_device_bytes_held() > before
        eng.synchronize()
        del eng
        gc.collect()
        assert lib.plda_device_bytes_held() == before


def test_api_edges(monkeypatch):
    from plda_amd import calibration as CB
    from plda_amd._native import PLDA_E_INVAL
    eng = _engine(monkeypatch)
    lib, h = eng._lib, eng._h
    rng = np.random.default_rng(10)
    m, nt = 20, 30
    es, ts = _labels(rng, m, nt, 4)
    Sh = rng.standard_normal((m, nt)).astype(np.float32)
    dS, des, dts, dO = _t(Sh), _t(es), _t(ts), _t(np.zeros((m, nt), np.float32))
    U, V, _ = _operands(rng, m, nt, 32, False)
    dU, dV = _t(U), _t(V)
    rec, fit = np.zeros(1, CB.RECORD_DTYPE), np.zeros(1, CB.FIT_DTYPE)
    R, F = C.c_void_p(rec.ctypes.data), C.c_void_p(fit.ctypes.data)
    vp = lambda t: C.c_void_p(t.data_ptr())                                        # noqa: E731
    pos, neg = np.float32([1.0, 2.0]), np.float32([-1.0, 0.5, 0.0])
    P, Q = C.c_void_p(pos.ctypes.data), C.c_void_p(neg.ctypes.data)
    bad = [
        lib.plda_calib_pass_matrix_dev(h, None, nt, m, nt, vp(des), vp(dts), 1.0, 0.0, 0.0, R),
        lib.plda_calib_pass_matrix_dev(h, vp(dS), nt, m, nt, None, vp(dts), 1.0, 0.0, 0.0, R),
        lib.plda_calib_pass_matrix_dev(h, vp(dS), nt, m, nt, vp(des), vp(dts), 1.0, 0.0, 0.0, None),
        lib.plda_calib_pass_matrix_dev(h, vp(dS), nt, 0, nt, vp(des), vp(dts), 1.0, 0.0, 0.0, R),
        lib.plda_calib_pass_matrix_dev(h, vp(dS), nt - 1, m, nt, vp(des), vp(dts), 1.0, 0.0, 0.0, R),
        lib.plda_calib_fit_matrix_dev(h, vp(dS), nt, m, nt, vp(des), vp(dts), 0.0, 0.0, 0, F),
        lib.plda_calib_fit_matrix_dev(h, vp(dS), nt, m, nt, vp(des), vp(dts), 1.0, 0.0, 0, F),
        lib.plda_calib_fit_matrix_dev(h, vp(dS), nt, m, nt, vp(des), vp(dts), float("nan"), 0.0, 0, F),
        lib.plda_calib_fit_matrix_dev(h, vp(dS), nt, m, nt, vp(des), vp(dts), 0.5, -1.0, 0, F),
        lib.plda_calib_fit_matrix_dev(h, vp(dS), nt, 0, nt, vp(des), vp(dts), 0.5, 0.0, 0, F),
        lib.plda_calib_fit_matrix_dev(h, vp(dS), nt, m, nt, vp(des), vp(dts), 0.5, 0.0, 0, None),
        lib.plda_calib_pass_lists(h, None, 2, Q, 3, 1.0, 0.0, 0.0, R),
        lib.plda_calib_pass_lists(h, P, 0, Q, 3, 1.0, 0.0, 0.0, R),
        lib.plda_calib_pass_lists(h, P, 2, Q, 3, 1.0, 0.0, 0.0, None),
        lib.plda_calib_fit_lists(h, P, 2, Q, 0, 0.5, 0.0, 0, F),
        lib.plda_calib_fit_lists(h, P, 2, Q, 3, 1.5, 0.0, 0, F),
        lib.plda_score_calib_pass_dev(h, None, None, 1, m, vp(dV), nt, None, None, vp(des), vp(dts), 1.0, 0.0, 0.0, R),
        lib.plda_score_calib_pass_dev(h, vp(dU), None, 0, m, vp(dV), nt, None, None, vp(des), vp(dts), 1.0, 0.0, 0.0, R),
        lib.plda_score_calib_pass_dev(h, vp(dU), None, 1, 0, vp(dV), nt, None, None, vp(des), vp(dts), 1.0, 0.0, 0.0, R),
        lib.plda_score_calib_fit_dev(h, vp(dU), None, 1, m, vp(dV), nt, None, None, None, vp(dts), 0.5, 0.0, 0, F),
        lib.plda_score_calib_fit_dev(h, vp(dU), None, 1, m, vp(dV), nt, None, None, vp(des), vp(dts), -0.1, 0.0, 0, F),
        lib.plda_affine_map_dev(h, None, nt, m, nt, 1.0, 0.0, vp(dO), nt),
        lib.plda_affine_map_dev(h, vp(dS), nt, m, nt, 1.0, 0.0, None, nt),
        lib.plda_affine_map_dev(h, vp(dS), nt, 0, nt, 1.0, 0.0, vp(dO), nt),
        lib.plda_affine_map_dev(h, vp(dS), nt - 1, m, nt, 1.0, 0.0, vp(dO), nt),
        lib.plda_affine_map_dev(h, vp(dS), nt, m, nt, 1.0, 0.0, vp(dO), nt - 1),
        lib.plda_calib_pass_matrix_dev(None, vp(dS), nt, m, nt, vp(des), vp(dts), 1.0, 0.0, 0.0, R),
    ]
    assert bad == [PLDA_E_INVAL] * len(bad), bad
    # one class only: every trial a target
    one = _t(np.zeros(m, np.int64)), _t(np.zeros(nt, np.int64))
    assert lib.plda_calib_pass_matrix_dev(h, vp(dS), nt, m, nt, vp(one[0]), vp(one[1]), 1.0, 0.0, 0.0, R) == PLDA_E_INVAL
    assert "at least one target" in eng._lib.plda_last_error(h).decode()
    assert int(rec["np"][0]) == m * nt and int(rec["nn"][0]) == 0          # the record is written all the same
    # and the handle still works
    got = CB.pass_from_matrix_dev(eng, dS.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr(), 1.0, 0.0, 0.0)
    _compare("after the edges", got, cm.pass_matrix(Sh, es, ts, 1.0, 0.0, 0.0))
    eng.synchronize()
    assert np.array_equal(dO.cpu().numpy(), np.zeros((m, nt), np.float32))   # no refused map wrote anything
