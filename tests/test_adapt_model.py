"""CPU: the host model of PLDA domain adaptation (tests/adapt_model.py) against itself -- Kaldi's update in Kaldi's order
of operations and the short form the engine computes are the same map; the oracle-free invariants of the update hold;
records about one pilot add; and the shift case that fixes the contract's choice of sums about the pilot."""
import numpy as np
import pytest

import adapt_model as AM


def _case(d, seed, scale=1.5, n=None):
    mean, T, psi = AM.synthetic_model(d, seed)
    n = n or 3 * d + 50
    x = AM.sample(mean, T, psi, n, seed + 1, scale=scale, offset=0.3 * np.ones(d))
    w = np.random.default_rng(seed + 2).random(n) + 0.1
    return mean, T, psi, AM.record(x, mean, w)


@pytest.mark.parametrize("d", [8, 200, 520])
@pytest.mark.parametrize("scales", [(0.3, 0.7, 1.0), (1.0, 0.0, 0.0), (0.0, 0.0, 0.5)])
def test_two_update_forms_agree(d, scales):
    """W', B' and the new psi of the two forms within 1e-12 relative (measured 1.4e-14)."""
    mean, T, psi, rec = _case(d, 100 + d)
    a = AM.update_kaldi(mean, T, psi, rec, *scales)
    b = AM.update_short(mean, T, psi, rec, *scales)
    assert AM.rel(b["W"], a["W"]) < 1e-12 and AM.rel(b["B"], a["B"]) < 1e-12
    assert AM.rel(b["psi"], a["psi"]) < 1e-12
    assert AM.rel(b["s"], a["s"]) < 1e-12
    assert np.array_equal(a["mean"], b["mean"])
    assert (a["s"] > 1.0).sum() > 0


@pytest.mark.parametrize("d", [8, 24, 200])
def test_total_covariance_gains_exactly_the_excess(d):
    """within_scale + between_scale = 1: in the basis where the old total covariance is the identity, the new total
    covariance has the eigenvalues max(s, 1)."""
    mean, T, psi, rec = _case(d, 7 + d, scale=1.2)
    out = AM.update_short(mean, T, psi, rec, 0.3, 0.7, 1.0)
    tm = T / np.sqrt(1.0 + psi)[:, None]
    lam = np.sort(np.linalg.eigvalsh(tm @ (out["W"] + out["B"]) @ tm.T))[::-1]
    assert np.abs(lam - np.maximum(out["s"], 1.0)).max() < 1e-8 * max(1.0, out["s"].max())
    assert 0 < (out["s"] > 1.0).sum()


@pytest.mark.parametrize("d", [8, 24, 200])
def test_zero_scales_move_only_the_mean(d):
    mean, T, psi, rec = _case(d, 31 + d)
    out = AM.update_kaldi(mean, T, psi, rec, 0.0, 0.0, 1.0)
    assert AM.rel(out["transform"].T @ out["transform"], T.T @ T) < 1e-8
    assert AM.rel(out["transform"].T @ (out["transform"] * out["psi"][:, None]), T.T @ (T * psi[:, None])) < 1e-8
    assert AM.rel(out["psi"], psi) < 1e-8
    assert np.abs(out["mean"] - mean).max() > 0.1


@pytest.mark.parametrize("d", [8, 24, 200])
def test_second_adaptation_on_the_same_rows_changes_nothing(d):
    """After an update with within_scale + between_scale = 1 the data no longer exceeds the model."""
    mean, T, psi = AM.synthetic_model(d, 5 + d)
    x = AM.sample(mean, T, psi, 3 * d + 50, 6 + d, scale=1.5, offset=0.3 * np.ones(d))
    one = AM.update_short(mean, T, psi, AM.record(x, mean))
    two = AM.update_short(one["mean"], one["transform"], one["psi"], AM.record(x, one["mean"]))
    assert AM.rel(two["psi"], one["psi"]) < 1e-8
    assert (two["s"] - 1.0).max() < 1e-8


def test_records_about_one_pilot_add():
    d, n = 24, 1000
    rng = np.random.default_rng(3)
    x, w, p = rng.standard_normal((n, d)) + 2.0, rng.random(n), rng.random(d)
    whole = AM.augmented(AM.record(x, p, w))
    both = AM.augmented(AM.merge(AM.record(x[:400], p, w[:400]), AM.record(x[400:], p, w[400:])))
    assert (np.abs(both - whole) <= 1e-12 * AM.record_bound(x, p, w)).all()


def test_shift_case_fixes_the_contract():
    """Offset 1e5, unit spread, D = 24, N = 4000: Kaldi's sums about 0 lose more than 1e-6 of the variance, the sums about a
    pilot near the data stay within 1e-10 of the long double result."""
    d, n = 24, 4000
    rng = np.random.default_rng(11)
    pilot = 1e5 + rng.random(d)
    x = pilot[None, :] + 0.5 + rng.standard_normal((n, d))
    exact = AM.centred_variance(AM.record(x, pilot, dtype=np.longdouble)).astype(np.float64)
    naive = AM.naive_variance(x)
    pilot_form = AM.centred_variance(AM.record(x, pilot))
    assert np.abs(naive - exact).max() > 1e-6
    assert np.abs(pilot_form - exact).max() < 1e-10 * np.abs(exact).max()


@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
def test_blend_endpoints(alpha):
    a, b = AM.synthetic_model(24, 1), AM.synthetic_model(24, 2)
    out = AM.blend(a, b, alpha, 0.25)
    Wa, Ba = AM.covariances(a[1], a[2])
    Wb, Bb = AM.covariances(b[1], b[2])
    Wn, Bn = AM.covariances(out["transform"], out["psi"])
    assert AM.rel(Wn, (1 - alpha) * Wa + alpha * Wb) < 1e-10 and AM.rel(Bn, (1 - alpha) * Ba + alpha * Bb) < 1e-10
    assert np.allclose(out["mean"], 0.75 * a[0] + 0.25 * b[0], rtol=1e-15)
    assert (np.diff(out["psi"]) <= 0).all()
