"""CPU: the minDCF definition (tests/mindcf_model.py) against a brute-force count, and the library's exported host step
(plda_min_dcf_step / plda_min_dcf_finish, pure functions) driven level by level with NumPy histograms against the
definition, bit for bit."""
import numpy as np
import pytest

import mindcf_model as mm


def _small_sets():
    rng = np.random.default_rng(7)
    sets = []
    for n_pos, n_neg, q in ((40, 160, None), (100, 100, 0.5), (3, 197, None), (60, 60, 0.25), (1, 1, None)):
        pos, neg = rng.normal(1.5, 1.0, n_pos), rng.normal(0.0, 1.0, n_neg)
        if q:
            pos, neg = np.round(pos / q) * q, np.round(neg / q) * q
        sets.append(("gauss%d_%d_%s" % (n_pos, n_neg, q), pos.astype(np.float32), neg.astype(np.float32)))
    sets.append(("signed_zeros", np.array([0.0, -0.0, 0.5, -0.0], np.float32), np.array([-0.0, 0.0, -1.0, 0.0, 0.25], np.float32)))
    sets.append(("targets_at_low_end", np.array([-5.0, -4.0, 1.0], np.float32), rng.normal(0, 1, 50).astype(np.float32)))
    sets.append(("non_targets_at_high_end", rng.normal(0, 1, 50).astype(np.float32), np.array([7.0, 8.0, 9.0, 0.0], np.float32)))
    sets.append(("separable", np.linspace(2.0, 3.0, 30).astype(np.float32), np.linspace(-1.0, 1.0, 90).astype(np.float32)))
    same = rng.normal(0, 1, 64).astype(np.float32)
    sets.append(("identical_lists", same.copy(), same.copy()))
    sets.append(("reversed", np.linspace(-3.0, -2.0, 20).astype(np.float32), np.linspace(1.0, 2.0, 20).astype(np.float32)))
    return sets


SMALL = _small_sets()


@pytest.mark.parametrize("name,pos,neg", SMALL, ids=[s[0] for s in SMALL])
def test_model_against_brute_force(name, pos, neg):
    assert len(pos) + len(neg) <= 200
    pts = mm.FIVE + ((0.3, 2.0, 5.0),)
    ref, bf = mm.model(pos, neg, pts), mm.brute(pos, neg, pts)
    for pt, r, (v, miss, fa, cut) in zip(pts, ref, bf):
        assert (r["miss"], r["fa"], r["cut"]) == (miss, fa, cut)
        assert r["min_dcf"] == min(v / min(pt[1] * pt[0], pt[2] * (1.0 - pt[0])), 1.0)
        if name == "separable":
            assert r["min_dcf"] == 0.0 and r["miss"] == 0 and r["fa"] == 0
        if name == "identical_lists":
            assert r["min_dcf"] == 1.0 and r["cut"] in (0, len(np.unique(mm.keys(pos))))
        if name == "signed_zeros":
            assert np.float64(r["threshold"]).tobytes() != np.float64(-0.0).tobytes()


def test_min_dcf_is_at_most_one():
    """min_dcf <= 1 always: the better of the two trivial cuts costs min(a, b) with a = c_miss * prior, b = c_fa * (1 - prior).
    The float64 expression alone misses that by one ulp -- the empty cut's value is (b * Nn) / Nn, which is one ulp above b on
    targets_at_low_end (Np = 3, Nn = 50) at the points (0.05, 1, 1) and (0.005, 10, 1): quotient 1.0000000000000002 -- so the
    definition reports min(quotient, 1); the sets here hold such a case, and the library's host step reports 1.0 on it too."""
    pts = mm.FIVE + ((0.3, 2.0, 5.0),)
    rounded_above = 0
    for name, pos, neg in SMALL:
        ref, bf = mm.model(pos, neg, pts), mm.brute(pos, neg, pts)
        got, _, _ = mm.refine(pos, neg, pts)
        for pt, r, g, (v, _, _, _) in zip(pts, ref, got, bf):
            assert r["min_dcf"] <= 1.0 and g["min_dcf"] <= 1.0, (name, pt, r["min_dcf"], g["min_dcf"])
            assert mm.same(r, g), (name, pt, r, g)
            rounded_above += v / min(pt[1] * pt[0], pt[2] * (1.0 - pt[0])) > 1.0
    assert rounded_above >= 1


def _check_refinement(pos, neg, pts, chunk=None):
    ref = mm.model(pos, neg, pts)
    got, survivors, _ = mm.refine(pos, neg, pts, slots_chunk=chunk)
    assert not isinstance(got, int), "host step failed: %r" % (got,)
    for r, g in zip(ref, got):
        assert mm.same(r, g), (r, g)
    # the survivors always contain the model's minimiser until a bin edge resolves it
    allk = np.unique(np.concatenate([mm.keys(pos), mm.keys(neg)]))
    for r in ref:
        if r["cut"] == 0:
            continue
        k = int(allk[r["cut"] - 1])
        nxt = int(allk[r["cut"]]) if r["cut"] < len(allk) else None
        for level in range(2):
            sh = mm.SHIFTS[level]
            if nxt is None or (nxt >> sh) != (k >> sh):
                break                                   # the largest key of its bin: the cut is this level's bin edge
            assert level < len(survivors) and (k >> sh) in [s[0] for s in survivors[level]], (level, hex(k))
    return survivors


TABLE = [
    ("llr_like_nist", (1, 20000, 2000000, 18, 9, -25, 14, None), mm.NIST),
    ("llr_like_five", (1, 20000, 2000000, 18, 9, -25, 14, None), mm.FIVE),
    ("znorm_like_nist", (2, 10000, 1000000, 6, 1.5, 0, 1, None), mm.NIST),
    ("znorm_like_five", (2, 10000, 1000000, 6, 1.5, 0, 1, None), mm.FIVE),
    ("one_in_200_seed0", (10, 10000, 2000000, 2.5, 1, 0, 1, None), mm.NIST),
    ("one_in_200_seed1", (11, 10000, 2000000, 2.5, 1, 0, 1, None), mm.NIST),
    ("one_in_200_seed2", (12, 10000, 2000000, 2.5, 1, 0, 1, None), mm.NIST),
    ("poor_nist", (3, 5000, 500000, 1, 1, 0, 1, None), mm.NIST),
    ("poor_five", (3, 5000, 500000, 1, 1, 0, 1, None), mm.FIVE),
    ("ties_nist", (4, 5000, 500000, 1, 1, 0, 1, 0.125), mm.NIST),
    ("ties_five", (4, 5000, 500000, 1, 1, 0, 1, 0.125), mm.FIVE),
]


@pytest.mark.parametrize("name,gen,pts", TABLE, ids=[t[0] for t in TABLE])
def test_host_step_reproduces_the_model_on_the_table(name, gen, pts):
    pos, neg = mm.gaussian_lists(*gen)
    _check_refinement(pos, neg, pts)


def test_host_step_on_the_flat_cost_set():
    pos, neg = mm.flat_cost_lists()
    survivors = _check_refinement(pos, neg, ((0.5, 1.0, 1.0),))
    assert len(survivors[0]) > 8                        # nothing to prune at level 0: what the several-launches path is for
    _check_refinement(neg, pos, ((0.5, 1.0, 1.0),))     # non-target first in each pair: the minimum is tied n times
    _check_refinement(pos, neg, ((0.5, 1.0, 1.0),), chunk=3)


def test_host_step_on_200_random_small_sets():
    rng = np.random.default_rng(2024)
    for case in range(200):
        n_pos, n_neg = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        mu, q = rng.uniform(0.0, 4.0), (None, 0.5, 0.0625)[case % 3]
        pos, neg = rng.normal(mu, 1.0, n_pos), rng.normal(0.0, 1.0, n_neg)
        if case % 7 == 0:
            pos, neg = pos * 1e-3, neg * 1e3            # scores spread over many octaves
        if q:
            pos, neg = np.round(pos / q) * q, np.round(neg / q) * q
        pts = tuple((float(rng.uniform(1e-3, 0.999)), float(rng.uniform(0.1, 10.0)), float(rng.uniform(0.1, 10.0)))
                    for _ in range(int(rng.integers(1, 9))))
        _check_refinement(pos.astype(np.float32), neg.astype(np.float32), pts, chunk=(None, 1, 5)[case % 3])


def test_host_step_refuses_what_the_device_call_refuses():
    from plda_amd import dcf as D
    pos, neg = mm.gaussian_lists(5, 50, 500, 2, 1, 0, 1)
    for bad, count in ((np.float32("nan"), 1), (np.float32("inf"), 1), (np.float32("-inf"), 1)):
        rc, _, state = mm.refine(np.append(pos, bad), neg, mm.NIST)
        assert rc == -1 and int(state[0]["nonfinite"]) == count
    hist = np.zeros((1, 2, 2048), np.uint64)
    hist[0, 1, 1000] = 5                                # targets only
    state = np.zeros(1, D.STATE_DTYPE)
    rc, _ = D.host_step(0, np.zeros(1, D.NODE_DTYPE), hist, mm.NIST, state, 2048)
    assert rc == -1 and int(state[0]["np"]) == 5 and int(state[0]["nn"]) == 0
    hist[0, 0, 900] = 7
    for pts in (((0.0, 1.0, 1.0),), ((1.0, 1.0, 1.0),), ((0.5, 0.0, 1.0),), ((0.5, 1.0, -1.0),), ((0.5, 1.0, 1.0),) * 9):
        if len(pts) > D.MAX_POINTS:
            with pytest.raises(ValueError):
                D.host_step(0, np.zeros(1, D.NODE_DTYPE), hist, pts, state, 2048)
        else:
            assert D.host_step(0, np.zeros(1, D.NODE_DTYPE), hist, pts, state, 2048)[0] == -1
    rc, nxt = D.host_step(0, np.zeros(1, D.NODE_DTYPE), hist, mm.NIST, state, 2048)
    assert rc == 0 and len(nxt) == 0                    # every bin holds one class: resolved at the edges


def test_min_dcf_never_exceeds_the_cost_at_any_threshold():
    """Property 2 of the definition, on the host: the counts at any threshold are those of some cut."""
    pos, neg = mm.gaussian_lists(6, 2000, 50000, 2, 1, 0, 1)
    ref = mm.model(pos, neg, mm.FIVE)
    rng = np.random.default_rng(1)
    for theta in rng.uniform(-3, 5, 20):
        miss, fa = int(np.sum(pos.astype(np.float64) < theta)), int(np.sum(neg.astype(np.float64) >= theta))
        for pt, r in zip(mm.FIVE, ref):
            act = (pt[1] * pt[0] * miss / len(pos) + pt[2] * (1.0 - pt[0]) * fa / len(neg)) / min(pt[1] * pt[0], pt[2] * (1.0 - pt[0]))
            assert r["min_dcf"] <= act
