"""CPU: the NumPy model of the VBx resegmentation (tests/vbx_model.py) against the published log-domain form and its own
invariants, the host wrappers' argument errors, and the conditions the GPU cases of tests/test_gpu_vbx.py rest on."""
import numpy as np
import pytest

import vbx_model as M


@pytest.mark.parametrize("shape", [(40, 8, 2, 3), (200, 32, 3, 10), (300, 128, 4, 64), (1000, 16, 4, 8)])
@pytest.mark.parametrize("pset", sorted(M.PARAMS))
def test_scaled_form_equals_the_log_domain_form(shape, pset):
    """gamma within 1e-8 wherever the log form stays finite; pi sums to 1; the ELBO does not decrease beyond rounding"""
    t, d, k, s = shape
    y, labels, _, phi = M.generate(t, d, k, s, 31 * t + d)
    fa, fb, p = M.PARAMS[pset]
    kw = dict(fa=fa, fb=fb, loop_prob=p, max_iters=10, epsilon=-np.inf)
    a = M.run(y, labels, phi, **kw)
    assert a["iters"] == 10 and np.isfinite(a["gamma"]).all() and np.isfinite(a["elbo"]).all()
    assert abs(a["pi"].sum() - 1.0) <= 1e-12 and (a["pi"] >= 0).all()
    assert np.max(np.abs(a["gamma"].sum(axis=1) - 1.0)) <= 1e-9
    steps = np.diff(a["elbo"])
    assert (steps >= -1e-9 * np.abs(a["elbo"][1:])).all(), steps
    b = M.run_log(y, labels, phi, **kw)
    n = b["iters"] if b["finite"] else b["iters"] - 1           # the iterations over which the log form stayed finite
    assert n >= 1
    if n < 10:
        a = M.run(y, labels, phi, **dict(kw, max_iters=n))
        b = M.run_log(y, labels, phi, **dict(kw, max_iters=n))
    assert np.max(np.abs(a["gamma"] - b["gamma"])) <= 1e-8
    assert np.max(np.abs(a["pi"] - b["pi"])) <= 1e-8
    assert np.max(np.abs(a["elbo"][:n] - b["elbo"][:n]) / np.abs(b["elbo"][:n])) <= 1e-10
    assert np.array_equal(a["labels"], b["labels"])


def test_one_initial_speaker_gives_gamma_one():
    y, labels, _, phi = M.generate(30, 6, 1, 1, 5)
    out = M.run(y, labels, phi, max_iters=5, epsilon=-np.inf)
    assert (out["gamma"] == 1.0).all() and out["pi"].tolist() == [1.0] and out["n_clusters"] == 1 and (out["labels"] == 0).all()


@pytest.mark.parametrize("name", ["257x130x4x12", "300x64x4x10", "600x48x5x16", "4096x32x4x8"])
def test_planted_speakers_are_recovered(name):
    r = M.reference(name)
    want, k = M.first_member_labels(r["spk"])
    assert r["f64"]["n_clusters"] == k and np.array_equal(r["f64"]["labels"], want)


def test_stop_rule_and_elbo_tail():
    y, labels, _, phi = M.generate(120, 12, 3, 6, 9)
    full = M.run(y, labels, phi, max_iters=20, epsilon=-np.inf)
    out = M.run(y, labels, phi, max_iters=20, epsilon=1e-4)
    n = out["iters"]
    assert 2 <= n < 20 and np.isnan(out["elbo"][n:]).all() and np.array_equal(out["elbo"][:n], full["elbo"][:n])
    assert out["elbo"][n - 1] - out["elbo"][n - 2] < 1e-4 and (np.diff(out["elbo"][:n - 1]) >= 1e-4).all()
    assert M.run(y, labels, phi, max_iters=1)["iters"] == 1


def test_first_member_labels():
    got, k = M.first_member_labels([5, 5, 2, 7, 2, 5])
    assert got.tolist() == [0, 0, 1, 2, 1, 0] and k == 3


def test_host_wrappers_reject_bad_arguments_before_any_device_work():
    """engine=None: a wrapper that touched the device before its checks would fail differently"""
    from plda_amd import diarize
    y, labels, _, phi = M.generate(10, 4, 2, 3, 1)
    off = np.asarray([0, 4, 10], np.int64)
    ok = dict(y=y, offsets=off, labels=labels, phi=phi)

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            diarize.vbx(None, **dict(ok, **kw))

    bad("Fa", Fa=0.0)
    bad("Fa", Fa=float("nan"))
    bad("Fb", Fb=-1.0)
    bad("loop_prob", loop_prob=1.0)
    bad("loop_prob", loop_prob=-0.1)
    bad("max_iters", max_iters=0)
    bad("offsets", offsets=np.asarray([1, 4, 10]))
    bad("segments", offsets=np.asarray([0, 4, 4, 10]))
    bad("segments", offsets=np.asarray([0, 10, 4]))
    bad("y must be", offsets=np.asarray([0, 4, 9]))
    bad("labels must lie", labels=np.where(np.arange(10) == 3, 64, labels))
    bad("labels must lie", labels=np.where(np.arange(10) == 3, -1, labels))
    bad("labels must hold", labels=labels[:9])
    ynan = y.copy()
    ynan[2, 1] = np.nan
    bad("non-finite", y=ynan)
    bad("phi", phi=phi[:3])
    bad("phi", phi=-phi)
    big = np.zeros((diarize.AHC_MAX + 1, 2))
    with pytest.raises(ValueError, match="segments"):
        diarize.vbx(None, big, np.asarray([0, len(big)]), np.zeros(len(big), np.int32))
    _, _, _, _, spk = diarize.vbx_args(y, off, labels, phi, 0.3, 17.0, 0.99, 40)
    assert spk.tolist() == [int(labels[:4].max()) + 1, int(labels[4:].max()) + 1]


def test_state_formula_and_boundary():
    lo, hi = M.lds_boundary()
    assert M.state_doubles(lo, 8, 16) <= M.LDS_DOUBLES < M.state_doubles(hi, 8, 16) and hi == lo + 1
    assert M.state_doubles(4096, 64, 128) > M.LDS_DOUBLES


@pytest.mark.parametrize("name", sorted(M.cases()))
def test_conditions_of_the_gpu_cases(name):
    """what makes 'labels must EQUAL the model's' and the parity band of tests/test_gpu_vbx.py well-posed, per case and
    parameter set used there"""
    t, d, k, s, _ = M.cases()[name]
    r = M.reference(name)
    a, b = r["f64"], r["ld"]
    assert int(r["labels"].max()) + 1 == s
    if k >= 2:
        assert a["n_clusters"] >= 2, "the model collapsed to one speaker"
    assert M.margin(a["gamma"]) >= 1e-6
    assert np.array_equal(a["labels"], b["labels"]) and a["n_clusters"] == b["n_clusters"]
    assert max(M.deviation(a, b)) <= 1e-9
    assert a["iters"] == M.ITERS and np.isfinite(a["elbo"]).all()


@pytest.mark.parametrize("name", M.STOP_CASES)
def test_stop_cases_have_a_well_separated_epsilon(name):
    r = M.reference(name)
    eps, want = M.stop_epsilon(r)
    assert eps > 0 and 2 <= want["iters"] < M.ITERS
    ld = M.run(r["y"], r["labels"], r["phi"], *r["params"], max_iters=M.ITERS, epsilon=eps, dtype=np.longdouble)
    assert ld["iters"] == want["iters"]
