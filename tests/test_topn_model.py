"""CPU: the host model of top-N selection (tests/topn_model.py) against a plain Python sort, the rank-N figures of
plda_amd/identify.py against hand-worked cases, the host form of the calibration map against exact rationals, and the
ctypes table."""
import struct
from fractions import Fraction

import numpy as np
import pytest

import topn_model as tm


def _key(x):
    """The key of one fp32 value, from its bits, in plain Python."""
    u = struct.unpack("<I", struct.pack("<f", x))[0]
    if u == 0x80000000:
        u = 0
    return (~u & 0xFFFFFFFF) if (u & 0x80000000) else (u | 0x80000000)


def _python_top_n(S, n, axis):
    lines = S if axis == 0 else S.T
    idx = np.empty((lines.shape[0], n), np.int64)
    for i, line in enumerate(lines):
        order = sorted(range(len(line)), key=lambda j: (-_key(float(line[j])), j))
        idx[i] = order[:n]
    return idx


def _matrices():
    rng = np.random.default_rng(0)
    yield "gaussian", rng.standard_normal((7, 13)).astype(np.float32)
    yield "ties", rng.integers(-2, 3, (9, 11)).astype(np.float32)
    z = np.zeros((5, 8), np.float32)
    z[rng.random((5, 8)) < 0.5] = -0.0
    yield "signed zeros", z
    mixed = rng.integers(-1, 2, (6, 10)).astype(np.float32)
    mixed[mixed == 0] = np.where(rng.random((mixed == 0).sum()) < 0.5, -0.0, 0.0)
    mixed[0, 3], mixed[2, 5], mixed[4, 1] = np.inf, -np.inf, np.float32(1e-42)
    yield "zeros, infinities, a denormal", mixed
    yield "one element", np.array([[3.5]], np.float32)


@pytest.mark.parametrize("axis", [0, 1])
def test_model_agrees_with_a_plain_sort(axis):
    for name, S in _matrices():
        length = S.shape[1 - axis]
        for n in sorted({min(k, length) for k in (1, 2, length // 2 or 1, length)}):
            scores, index = tm.top_n(S, n, axis)
            assert scores.dtype == np.float32 and index.dtype == np.int64
            assert scores.shape == index.shape == (S.shape[axis], n)
            assert np.array_equal(index, _python_top_n(S, n, axis)), (name, n)
            lines = S if axis == 0 else S.T
            picked = np.take_along_axis(lines, index, axis=1)
            assert np.array_equal(scores.view(np.uint32), picked.view(np.uint32)), (name, n)   # bit for bit: -0.0 stays -0.0


def test_model_treats_signed_zeros_as_equal_and_keeps_their_bits():
    S = np.array([[-0.0, 0.0, -1.0, 0.0, -0.0]], np.float32)
    scores, index = tm.top_n(S, 4, 0)
    assert index.tolist() == [[0, 1, 3, 4]]
    assert np.signbit(scores[0]).tolist() == [True, False, False, True]
    assert tm.score_key(np.array([-0.0], np.float32))[0] == tm.score_key(np.array([0.0], np.float32))[0]


def test_key_is_monotone_over_all_classes_of_values():
    v = np.array([-np.inf, -3.0e38, -1.0, -1e-42, -0.0, 1e-42, 1.0, 3.0e38, np.inf], np.float32)
    k = tm.score_key(v).astype(np.int64)
    assert (np.diff(k) > 0).all()
    assert [int(x) for x in tm.score_key(v)] == [_key(float(x)) for x in v]


def test_rank_rates_and_cmc_hand_worked():
    from plda_amd import identify
    ids = np.array([[7, 3, 9],      # truth 7: rank 1
                    [4, 5, 6],      # truth 6: rank 3
                    [1, 2, 3],      # truth 8: absent
                    [2, 2, 5]])     # truth 2: rank 1 (the first hit counts)
    truth = np.array([7, 6, 8, 2])
    curve = identify.cmc(ids, truth)
    assert curve.dtype == np.float64 and curve.tolist() == [0.5, 0.5, 0.75]
    assert identify.rank_rates(ids, truth, ranks=(1, 3)) == {1: 0.5, 3: 0.75}
    assert identify.rank_rates(ids[:, :1], truth, ranks=(1,)) == {1: 0.5}
    with pytest.raises(ValueError, match="outside 1 ... n = 3"):
        identify.rank_rates(ids, truth)                      # the default ranks ask for rank 5 of 3 columns
    with pytest.raises(ValueError, match="true id of each of the 4 lines"):
        identify.cmc(ids, truth[:3])
    perfect = np.arange(12).reshape(12, 1) + np.zeros((1, 10), np.int64)
    assert identify.rank_rates(perfect, np.arange(12)) == {1: 1.0, 5: 1.0, 10: 1.0}


def test_host_affine_map_is_the_fused_one():
    """affine_f32 against exact rationals, on values built to sit at fp32 rounding midpoints of a * s + b (where the unfused
    fp64 product decides wrongly) as well as on ordinary ones."""
    from plda_amd import identify
    rng = np.random.default_rng(3)
    s = (rng.standard_normal(4000) * 30).astype(np.float32)
    s[:5] = [0.0, -0.0, np.inf, -np.inf, np.float32(1e-42)]
    cases = [(0.1, 3.0), (1.0 + 2.0 ** -30, 0.0), (3.0 + 2.0 ** -24 + 2.0 ** -52, -7.25), (1e-3, 1e3)]
    for a, b in cases:
        got = identify.affine_f32(a, s, b)
        assert got.dtype == np.float32 and got.shape == s.shape
        for i in range(s.shape[0]):
            if not np.isfinite(s[i]):
                assert got[i] == np.float32(a * float(s[i]) + b)
                continue
            exact = Fraction(a) * Fraction(float(s[i])) + Fraction(b)
            want = np.float32(float(exact))
            assert got[i] == want, (a, b, float(s[i]))
    # a = 1 + 2^-30 on s = 1 + 2^-23: the exact product is 1 + 2^-23 + 2^-30 + 2^-53, whose last term the fp64 product drops
    # (a tie, to even).  b cancels all but 2^-28 + 2^-52, the midpoint of two fp32 values: unfused, the sum IS that midpoint
    # and rounds to even (2^-28); fused, it lies 2^-53 above it and rounds up
    a = 1.0 + 2.0 ** -30
    b = -(1.0 + 2.0 ** -23 + 2.0 ** -30) + (2.0 ** -28 + 2.0 ** -52)
    s1 = np.array([1.0 + 2.0 ** -23], np.float32)
    assert np.float32(a * float(s1[0]) + b) == np.float32(2.0 ** -28)
    exact = Fraction(a) * Fraction(float(s1[0])) + Fraction(b)
    assert exact == Fraction(1, 2 ** 28) + Fraction(1, 2 ** 52) + Fraction(1, 2 ** 53)
    assert identify.affine_f32(a, s1, b)[0] == np.float32(2.0 ** -28 + 2.0 ** -51)


def test_ctypes_table_holds_the_new_entry_points():
    from plda_amd import _native
    for name in ("plda_topn_matrix_dev", "plda_score_topn_dev", "plda_score_topn"):
        assert name in _native.SIGNATURES
    assert len(_native.SIGNATURES["plda_score_topn_dev"][1]) == len(_native.SIGNATURES["plda_score_topn"][1]) == 17
    assert len(_native.SIGNATURES["plda_topn_matrix_dev"][1]) == 9
