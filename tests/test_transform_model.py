"""CPU: the rule K4's device tests use (tests/transform_model.py) is sound and has power.

  sound    a NumPy fp64 evaluation of the offset form -- the device's arithmetic in another summation order -- stays within the
           forward bound B of the longdouble model and within the normaliser residual's bound, with means of size 0, 1, 1e3
           and 1e6 (the bound is derived for any order, so a second evaluation far below it says the rule does not rest on luck);
  power    every planted fault of transform_model.offset_form is rejected.
Worst figures of the sound cases here: deviation 0.12 B (Din = 1), residual 4.2 u."""
import numpy as np
import pytest

import transform_model as M

SHAPES = [(1, 1), (7, 7), (33, 17), (200, 150), (512, 512), (520, 520)]
MEANS = [0.0, 1.0, 1e3, 1e6]
R = 67


def _case(din, dout, mean_size, seed=0):
    rng = np.random.default_rng([din, dout, int(mean_size), seed])
    mean, T, psi = M.make_model(rng, din, dout, mean_size)
    x = mean[None, :] + rng.standard_normal((R, din))
    n = rng.integers(1, 9, R).astype(np.int32)
    n[1::2] = np.where(n[1::2] == n[0::2][:len(n[1::2])], n[1::2] + 1, n[1::2])       # neighbours differ
    return mean, T, psi, x, n


def test_longdouble_has_a_64_bit_significand():
    assert M.longdouble_is_extended(), "np.longdouble is no wider than fp64 here: the model would restate the device"


@pytest.mark.parametrize("mean_size", MEANS)
@pytest.mark.parametrize("din,dout", SHAPES)
def test_numpy_offset_form_is_within_the_bound(din, dout, mean_size):
    mean, T, psi, x, n = _case(din, dout, mean_size)
    for counts in (3, n):
        ref = M.model(T, mean, psi, x, counts)
        M.assert_well_posed(ref)
        fig = M.assert_rule(M.offset_form(T, mean, psi, x, counts), ref, psi, counts, "NumPy fp64")
        print("Din %d Dout %d |mean| %g: deviation %.3g B, residual %.2f u" % (din, dout, mean_size, fig["dev"], fig["rho"]))
        assert fig["dev"] <= 0.5 and fig["rho"] <= 12          # far below: the rule does not rest on luck


def test_the_bound_grows_with_the_mean():
    """B / |out| is linear in |mean| / spread: what the offset form costs"""
    rel = []
    for mean_size in (1.0, 1e3, 1e6):
        mean, T, psi, x, n = _case(200, 150, mean_size)
        ref = M.model(T, mean, psi, x, 1)
        rel.append(float(np.median(ref["B"] / np.abs(ref["out"]))))
    assert 100 < rel[1] / rel[0] < 1000 * 1.5 and 500 < rel[2] / rel[1] < 1500, rel


def _rejected(fault, din, dout, mean_size):
    mean, T, psi, x, n = _case(din, dout, mean_size, seed=1)
    ref = M.model(T, mean, psi, x, n)
    M.assert_rule(M.offset_form(T, mean, psi, x, n), ref, psi, n, "no fault")
    try:
        M.assert_rule(M.offset_form(T, mean, psi, x, n, fault=fault), ref, psi, n, fault)
    except AssertionError as e:
        return str(e)
    return None


_FAULTS = [("kstep", 7, 7), ("kstep", 33, 17), ("kstep", 130, 128), ("kstep", 211, 208), ("kstep", 513, 513),
           ("neighbour", 1, 1), ("neighbour", 7, 7), ("neighbour", 200, 150), ("neighbour", 512, 512),
           ("offset16", 33, 17), ("offset16", 200, 150), ("offset16", 520, 520),
           ("weight", 7, 7), ("weight", 200, 150), ("weight", 512, 512)]


@pytest.mark.parametrize("fault,din,dout,mean_size", [f + (m,) for f in _FAULTS for m in MEANS
                                                      if not (f[0] == "offset16" and m == 0.0)])      # (a zero mean has no offset to leave out)
def test_planted_faults_are_rejected(fault, din, dout, mean_size):
    why = _rejected(fault, din, dout, mean_size)
    assert why, "the rule accepts the fault %r at Din %d Dout %d |mean| %g" % (fault, din, dout, mean_size)


@pytest.mark.parametrize("mean_size", MEANS)
@pytest.mark.parametrize("din,dout", [(1, 1), (7, 7), (33, 17), (64, 64), (200, 64)])
def test_a_factor_off_by_3e_14_is_rejected_by_the_residual(din, dout, mean_size):
    """one Newton step short in the refinement of rsq: the residual must see it at every Dout <= 64 (on offset data nothing else
    does: it is far inside B there)"""
    mean, T, psi, x, n = _case(din, dout, mean_size, seed=1)
    clean = M.rho(M.offset_form(T, mean, psi, x, n), psi, n)
    faulty = M.rho(M.offset_form(T, mean, psi, x, n, fault="f"), psi, n)
    assert clean.max() <= M.rho_bound(dout) and faulty.min() > M.rho_bound(dout), (float(clean.max() / M.U), float(faulty.min() / M.U))
    assert _rejected("f", din, dout, mean_size)


def test_the_fp64_bound_agrees_with_the_longdouble_one():
    mean, T, psi, x, n = _case(200, 150, 1e3)
    ref = M.model(T, mean, psi, x, n)
    out, B, rel_s = M.bound_fp64(T, mean, psi, x, n)
    assert (B >= ref["B"].astype(np.float64)).all() and (B <= ref["B"].astype(np.float64) * (1 + 1e-8)).all()


def test_pool_spread_and_representatives():
    """copies of a pool entry reach every position mod 16, 64 and 128 of a launch, and a planted position-dependent fault is caught"""
    rng = np.random.default_rng(3)
    r = 128 * M.POOL
    idx = M.spread_index(rng, r)
    for e in (0, 17, 60):
        pos = np.nonzero(idx == e)[0]
        for m in (16, 64, 128):
            assert len(set(pos % m)) == m
    plan = {"main_rows": 4096, "main_block": 128, "tail_rows": r - 4096, "tail_block": 32}
    got = rng.standard_normal((M.POOL, 5))[idx]
    rows, entries = M.assert_copies_identical(got, idx, plan)
    assert len(rows) == 2 * M.POOL and (idx[rows] == entries).all() and sorted(entries[:M.POOL]) == list(range(M.POOL))
    got[5000, 3] = np.nextafter(got[5000, 3], 9.0)
    with pytest.raises(AssertionError, match="row 5000"):
        M.assert_copies_identical(got, idx, plan)
