"""CPU tests of the host model of the fp32 trials GEMM (tests/fp32_chain.py).

`fma32` against exact rational arithmetic; the chain against a scalar chain of exact fmas; the rigorous
budget against the fp64 value; and the bit check that tests/test_gpu_score_model.py applies to the GPU's
scores, shown to REJECT each of the ways a kernel could be subtly wrong (k order, bias placement, a lost
column, truncated operands, r' summed in fp32, a bucket off by one, bf16x2 in place of bf16x3).  Needs no GPU.
"""
from fractions import Fraction

import numpy as np
import pytest

import fp32_chain as fc


# ------------------------------------------------------------------------------------------ fma32
def _rn32_exact(q):
    """The fp32 value nearest to the rational q (ties to even)."""
    f = np.float32(float(q))
    best = None
    for c in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
        dist = abs(Fraction(float(c)) - q)
        key = (dist, int(np.array(c, np.float32).view(np.uint32)) & 1)
        if best is None or key < best[0]:
            best = (key, c)
    return np.float32(best[1])


def _fma_exact(a, b, c):
    return _rn32_exact(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def _adversarial():
    """(a, b, c) triples where a double-rounded or carelessly emulated fma goes wrong."""
    one = np.float32(1.0)
    ulp = np.float32(2.0 ** -23)
    cases = [
        # a*b + c lands exactly on an fp32 midpoint in fp64, with an error term below it: double rounding
        (np.float32((1 + 2896 * 2.0 ** -23) * 2.0 ** -24), np.float32(1 - 2895 * 2.0 ** -23), one),
        (one + ulp, one + 2 * ulp, np.float32(2.0 ** -60)),
        (one + ulp, one - ulp / 2, np.float32(-2.0 ** -70)),
        (np.float32(3.0), np.float32(1 + 2.0 ** -22), np.float32(2.0 ** -24 * 3 + 2.0 ** -80)),
        # exact midpoints (ties to even, both directions)
        (one, one, np.float32(2.0 ** -24)),
        (one + ulp, one, np.float32(2.0 ** -24)),
        (np.float32(-1.0), one + ulp, np.float32(-2.0 ** -24)),
        # heavy cancellation
        (one + ulp, one - ulp, np.float32(-1.0)),
        (np.float32(1.0 / 3), np.float32(3.0), np.float32(-1.0)),
        (np.float32(12345.678), np.float32(0.0001), np.float32(-1.2345678)),
        # subnormal results and operands
        (_f32(0x00000003), np.float32(0.5), np.float32(0.0)),
        (_f32(0x00800000), np.float32(0.75), _f32(0x80000001)),
        (np.float32(2.0 ** -75), np.float32(2.0 ** -75), _f32(0x00000001)),
        (np.float32(2.0 ** -70), np.float32(-2.0 ** -70), _f32(0x00400000)),
        (_f32(0x00000001), np.float32(0.5), np.float32(0.0)),          # 2^-150: a tie at zero
        (_f32(0x00000003), np.float32(0.5), _f32(0x80000000)),
        # large magnitude next to a tiny one
        (np.float32(1e30), np.float32(1e-30), np.float32(1e-38)),
        (np.float32(3e38), np.float32(1.0), _f32(0x00000001)),
        (np.float32(1e20), np.float32(1e18), np.float32(-1e38)),
        (np.float32(2.0 ** 100), np.float32(2.0 ** -100), np.float32(2.0 ** -48)),
    ]
    return [tuple(np.float32(v) for v in t) for t in cases]


def test_fma32_adversarial_matches_exact():
    for a, b, c in _adversarial():
        got = fc.fma32(np.array([a]), np.array([b]), np.array([c]))[0]
        ref = _fma_exact(a, b, c)
        assert got.view(np.uint32) == ref.view(np.uint32) or (got == ref == 0), (a, b, c, got, ref)


def test_fma32_catches_double_rounding():
    """a b + c = 1 + 2^-24 + 2^-57.8 (scaled by 2^e, either sign): fp64 rounds it onto the fp32 midpoint
    1 + 2^-24, and fp32 then rounds that to even (1); the exact value lies above the midpoint (1 + 2^-23).
    The plain fp64 evaluation gets it wrong, fma32 does not."""
    a1 = np.float32(1 + 2896 * 2.0 ** -23)          # a1 b1 = 1 + 4688 2^-46
    b1 = np.float32(1 - 2895 * 2.0 ** -23)
    e = np.arange(-100, 101, 7)
    sgn = np.where(e % 2 == 0, 1.0, -1.0)
    a = (a1 * 2.0 ** -24 * 2.0 ** e * sgn).astype(np.float32)
    b = np.full(e.shape, b1, np.float32)
    c = (2.0 ** e * sgn).astype(np.float32)
    naive = (a.astype(np.float64) * b + c).astype(np.float32)
    got = fc.fma32(a, b, c)
    ref = np.array([_fma_exact(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got, ref)
    assert np.array_equal(np.abs(ref), (np.float32(1 + 2.0 ** -23) * 2.0 ** e).astype(np.float32))
    assert (naive != ref).all()


@pytest.mark.parametrize("scale", ["unit", "wide", "subnormal"])
def test_fma32_random_matches_exact(scale):
    rng = np.random.default_rng({"unit": 2, "wide": 3, "subnormal": 4}[scale])
    n = 4000
    if scale == "unit":
        a, b, c = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    elif scale == "wide":
        a, b, c = ((rng.standard_normal(n) * 2.0 ** rng.integers(-60, 60, n)).astype(np.float32) for _ in range(3))
    else:
        a = (rng.standard_normal(n) * 2.0 ** rng.integers(-80, -60, n)).astype(np.float32)
        b = (rng.standard_normal(n) * 2.0 ** rng.integers(-80, -60, n)).astype(np.float32)
        c = (rng.standard_normal(n) * 2.0 ** -140).astype(np.float32)
    got = fc.fma32(a, b, c)
    ref = np.array([_fma_exact(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got, ref)


# ------------------------------------------------------------------------------------------ the chain
def _model(d, seed=3, lo=0.05, hi=4.05):
    rng = np.random.default_rng(seed)
    return np.sort(lo + rng.random(d) * (hi - lo))[::-1].copy()


def _case(d=200, m=48, nt=40, n=7, seed=11, **kw):
    rng = np.random.default_rng(seed)
    psi = _model(d)
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    return psi, U, V, fc.operands(psi, U, V, n, **kw)


def test_kernel_order_is_a_permutation():
    for kg in (8, 16, 200, 2048):
        o = fc.kernel_order(kg)
        assert sorted(o) == list(range(kg + 2)) and list(o[:4]) == [0, 1, 2, 6]


def test_chain_matches_scalar_exact_chain():
    """The vectorised chain is the k-ordered chain of exactly rounded fmas (scalar, Fraction-based)."""
    _, _, _, op = _case(d=33, m=5, nt=4)
    got = fc.chain(op.A32, op.B32)
    order = fc.kernel_order(op.Kg)
    for i in range(op.A32.shape[0]):
        for j in range(op.B32.shape[0]):
            acc = np.float32(0.0)
            for k in order:
                acc = _fma_exact(op.A32[i, k], op.B32[j, k], acc)
            assert got[i, j] == acc, (i, j)


def test_operands_match_plain_llr():
    """The operands contract to the fp64 GEMM form of the LLR, all three forms."""
    rng = np.random.default_rng(5)
    d, m, nt = 24, 30, 20
    psi = _model(d)
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    counts = rng.integers(1, 6, m).astype(np.int32)
    counts[:5] = [1, 2, 3, 4, 5]

    def llr(u, n, v):
        den = n * psi + 1.0
        c, var = n * psi / den, 1.0 + psi / den
        return -0.5 * np.sum(np.log(var) - np.log(1 + psi) + (v - c * u) ** 2 / var - v * v / (1 + psi))

    ref = np.array([[llr(U[i], counts[i], V[j]) for j in range(nt)] for i in range(m)])
    for form in ("buckets", "depth2d"):
        op = fc.operands(psi, U, V, counts, form=form)
        ii, jj = fc.sample_pairs(m, nt, 10 ** 9)
        assert np.allclose(fc.exact(op, (ii, jj)), ref.ravel(), rtol=1e-12, atol=1e-10), form
    ref3 = np.array([[llr(U[i], 3, V[j]) for j in range(nt)] for i in range(m)])
    op = fc.operands(psi, U, V, 3)
    assert np.allclose(fc.exact(op, fc.sample_pairs(m, nt, 10 ** 9)), ref3.ravel(), rtol=1e-12, atol=1e-10)


@pytest.mark.parametrize("form", ["uniform", "buckets", "depth2d"])
@pytest.mark.parametrize("zn", [False, True])
def test_chain_within_budget(form, zn):
    rng = np.random.default_rng(6)
    d, m, nt = 65, 40, 33
    psi = _model(d, lo=1e-6, hi=1e4)
    U, V = rng.standard_normal((m, d)) * 2, rng.standard_normal((nt, d)) * 2
    n = 4 if form == "uniform" else rng.integers(1, 9, m).astype(np.int32)
    zm = zs = None
    if zn:
        zm, zs = rng.standard_normal(m) * 10, rng.random(m) * 5 + 0.1
        zs[::7] = 0.0
    op = fc.operands(psi, U, V, n, zm, zs, form=form)
    pairs = fc.sample_pairs(m, nt, 10 ** 9)
    err = np.abs(fc.chain(op.A32, op.B32, pairs).astype(np.float64) - fc.exact(op, pairs))
    assert (err <= fc.budget(op, pairs)).all()
    assert (fc.allowance(op, pairs) < fc.budget(op, pairs)).all()


# ------------------------------------------------------------------------------------------ mutants
def _rejects(got, op, pairs):
    ok, frac, ulp = fc.check(got, fc.chain(op.A32, op.B32, pairs), fc.allowance(op, pairs))
    return not ok


def test_faithful_chain_passes():
    _, _, _, op = _case()
    pairs = fc.sample_pairs(op.A32.shape[0], op.B32.shape[0], 10 ** 9)
    ok, frac, ulp = fc.check(fc.chain(op.A32, op.B32, pairs), fc.chain(op.A32, op.B32, pairs), fc.allowance(op, pairs))
    assert ok and frac == 1.0 and ulp == 0


@pytest.mark.parametrize("mutant", ["reversed", "sequential", "blocked4", "bias_last", "drop_column"])
def test_order_mutants_rejected(mutant):
    _, _, _, op = _case()
    pairs = fc.sample_pairs(op.A32.shape[0], op.B32.shape[0], 10 ** 9)
    order = list(fc.kernel_order(op.Kg))
    if mutant == "reversed":
        order = order[:2] + order[2:][::-1]
    elif mutant == "sequential":
        order = list(range(op.Kg + 2))
    elif mutant == "blocked4":        # whole k-quads in turn: 8p..8p+3, then 8p+4..8p+7
        order = [0, 1] + [2 + 8 * p + 4 * h + t for p in range(op.Kg // 8) for h in range(2) for t in range(4)]
    elif mutant == "bias_last":
        order = order[2:] + order[:2]
    else:
        order = [k for k in order if k != 2 + 100]
    assert _rejects(fc.chain(op.A32, op.B32, pairs, order), op, pairs), mutant


def test_truncated_operands_rejected():
    psi, U, V, op = _case()
    pairs = fc.sample_pairs(op.A32.shape[0], op.B32.shape[0], 10 ** 9)
    bad = fc.operands(psi, U, V, 7, rnd=fc.round_trunc)
    assert _rejects(fc.chain(bad.A32, bad.B32, pairs), op, pairs)


@pytest.mark.parametrize("form", ["uniform", "buckets", "depth2d"])
def test_r_in_fp32_rejected(form):
    rng = np.random.default_rng(9)
    psi = _model(200)
    U, V = rng.standard_normal((48, 200)), rng.standard_normal((40, 200))
    n = 7 if form == "uniform" else rng.integers(1, 6, 48).astype(np.int32)
    op = fc.operands(psi, U, V, n, form=form)
    bad = fc.operands(psi, U, V, n, form=form, r_fp32=True)
    pairs = fc.sample_pairs(48, 40, 10 ** 9)
    assert _rejects(fc.chain(bad.A32, bad.B32, pairs), op, pairs)


@pytest.mark.parametrize("values,g", [([1, 2, 3, 4, 5], 1), ([1, 4094, 4095], 1), ([200, 201], 0)])
def test_bucket_off_by_one_rejected(values, g):
    rng = np.random.default_rng(10)
    d, m, nt = 200, 60, 40
    psi = _model(d)
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    counts = np.asarray(values, np.int32)[rng.integers(0, len(values), m)]
    counts[:len(values)] = values
    op = fc.operands(psi, U, V, counts)
    assert op.form == "buckets"
    bad = fc.operands(psi, U, V, counts, swap_bucket=g)
    pairs = fc.sample_pairs(m, nt, 10 ** 9)
    assert _rejects(fc.chain(bad.A32, bad.B32, pairs), op, pairs)


def test_allowance_is_tight_against_score_tol():
    """The non-bit-identical allowance is far inside the suite's score_tol on these operands."""
    from conftest import score_tol
    psi, U, V, op = _case()
    pairs = fc.sample_pairs(op.A32.shape[0], op.B32.shape[0], 10 ** 9)
    ex = fc.exact(op, pairs)
    assert (fc.allowance(op, pairs) <= 0.1 * score_tol(ex)).all()


# ------------------------------------------------------------------------------------------ bf16x3
def _bf16_check(got, op, pairs):
    """The GPU test's bf16x3 criterion: max error within the split-model bound, RMS within 2x the fp32 chain's."""
    ex = fc.exact(op, pairs)
    err = got.astype(np.float64) - ex
    ref_rms = fc.rms(fc.chain(op.A32, op.B32, pairs).astype(np.float64) - ex)
    return bool((np.abs(err) <= fc.bf16x3_bound(op, pairs)).all()) and fc.rms(err) <= 2.0 * ref_rms


def test_split3_is_exact_to_24_bits():
    rng = np.random.default_rng(12)
    x = (rng.standard_normal(10000) * 2.0 ** rng.integers(-30, 30, 10000)).astype(np.float32)
    x0, x1, x2 = fc.split3(x)
    assert np.array_equal((x0.astype(np.float64) + x1 + x2), x.astype(np.float64))


def test_bf16x3_passes_and_bf16x2_rejected():
    _, _, _, op = _case(d=200, m=24, nt=20)
    pairs = fc.sample_pairs(24, 20, 10 ** 9)
    assert _bf16_check(fc.bf16x3_emulate(op, pairs), op, pairs)
    assert not _bf16_check(fc.bf16x3_emulate(op, pairs, kept=fc.KEPT2), op, pairs)
