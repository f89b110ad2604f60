"""CPU: the NumPy model of the speaker clustering (tests/ahc_model.py) is what the contract in include/plda_hip.h says -- checked
against scipy's average linkage on tie-free data, on hand-worked tie cases, and against its own definitional form -- and
plda_amd.diarize.cut replays a merge record to exactly what a run with those arguments gives.  The GPU tests
(tests/test_gpu_ahc.py) then compare the device with this model for equality."""
import numpy as np
import pytest

import ahc_model as M


def _same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


@pytest.mark.parametrize("n", [2, 3, 17, 64, 65, 130])
def test_model_matches_scipy_average_linkage(n):
    """Heights within 1e-12 relative (a summation-order bound: scipy updates means by Lance-Williams, the model keeps sums),
    merged sizes identical, partitions at 1, 2 and 5 clusters identical to fcluster(maxclust)."""
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    S = M.gaussian(n, 100 + n)
    c = M.costs(S)
    shift = 1.0 - c[~np.eye(n, dtype=bool)].min()          # scipy's distances must be non-negative
    iu = np.triu_indices(n, 1)
    Z = hier.linkage((c + shift)[iu], method="average")
    labels, k, ma, mb, mc = M.cluster_one(S)
    assert k == 1 and (ma >= 0).all()
    np.testing.assert_allclose(mc + shift, Z[:, 2], rtol=1e-12, atol=0)
    size = np.ones(n, np.int64)
    for i in range(n - 1):
        size[ma[i]] += size[mb[i]]
        assert size[ma[i]] == int(Z[i, 3])
    for want in (1, 2, 5):
        if want > n:
            continue
        got = M.cluster_one(S, None, want)[0]
        assert _same_partition(got, hier.fcluster(Z, want, "maxclust"))


@pytest.mark.parametrize("family", ["gaussian", "integers", "zeros", "equal", "chain", "chain_reverse"])
@pytest.mark.parametrize("n", [1, 2, 7, 33])
def test_working_model_equals_the_definition(family, n):
    S = {"gaussian": lambda: M.gaussian(n, n), "integers": lambda: M.integers(n, n), "zeros": lambda: M.signed_zeros(n, n),
         "equal": lambda: M.all_equal(n), "chain": lambda: M.chain(n), "chain_reverse": lambda: M.chain(n, True)}[family]()
    for thr, minc in ((None, 1), (0.0, 1), (-0.5, 3), (None, n), (5.0, 1)):
        fast = M.cluster_one(S, thr, minc)
        slow = M.cluster_one_definition(S, thr, minc)
        for f, s in zip(fast, slow):
            assert np.array_equal(np.asarray(f), np.asarray(s))
        assert np.array_equal(np.signbit(fast[4]), np.signbit(slow[4]))


def test_all_scores_equal_merges_into_slot_zero_in_index_order():
    """every v is equal at every step (sum = -s * size(a) * size(b)): the order (a, b) alone decides -- (0, 1), (0, 2), ..."""
    n = 6
    labels, k, ma, mb, mc = M.cluster_one(M.all_equal(n, 0.5))
    assert k == 1 and labels.tolist() == [0] * n
    assert ma.tolist() == [0] * (n - 1) and mb.tolist() == list(range(1, n))
    assert mc.tolist() == [-0.5] * (n - 1)


def test_integer_scores_hand_worked():
    """S (symmetric), costs c = -S:          step 1: the minimum -2 is shared by (0, 2) and (1, 3): (0, 2) wins on a.
         0   1   2   3                       sums: (0,1) = -1 + 0 = -1, (0,3) = 1 + 2 = 3 -> v(0,1) = -0.5, v(0,3) = 1.5
    0    .   1   2  -1                       step 2: (1, 3) at -2.  sum(0,1) = -1 + 3 = 2 over 2 x 2 pairs: v = 0.5
    1    1   .   0   2                       step 3: (0, 1) at 0.5
    2    2   0   .  -2
    3   -1   2  -2   ."""
    S = np.array([[0, 1, 2, -1], [1, 0, 0, 2], [2, 0, 0, -2], [-1, 2, -2, 0]], np.float32)
    labels, k, ma, mb, mc = M.cluster_one(S)
    assert (ma.tolist(), mb.tolist(), mc.tolist()) == ([0, 1, 0], [2, 3, 1], [-2.0, -2.0, 0.5])
    # a score threshold of 0: the last merge (average score -0.5) is refused
    labels, k, ma, mb, mc = M.cluster_one(S, 0.0)
    assert k == 2 and labels.tolist() == [0, 1, 0, 1]
    assert (ma.tolist(), mb.tolist()) == ([0, 1, -1], [2, 3, -1]) and mc[2] == np.inf
    # a count of 3 stops after the first
    assert M.cluster_one(S, None, 3)[0].tolist() == [0, 1, 0, 2]


def test_signed_zeros_compare_equal():
    """c(0, 1) = +0.0 and c(0, 2) = c(1, 2) = -0.0: were -0.0 < +0.0 the pair (0, 2) would go first; they are equal, so (0, 1)
    does, and its recorded cost keeps its own sign"""
    pz, nz = np.float32(0.0), np.float32(-0.0)
    S = np.array([[0, nz, pz], [nz, 0, pz], [pz, pz, 0]], np.float32)
    c = M.costs(S)
    assert not np.signbit(c[0, 1]) and np.signbit(c[0, 2]) and np.signbit(c[1, 2])
    labels, k, ma, mb, mc = M.cluster_one(S)
    assert (ma.tolist(), mb.tolist()) == ([0, 0], [1, 2])
    assert mc[0] == 0.0 and not np.signbit(mc[0])
    assert mc[1] == 0.0 and np.signbit(mc[1])            # (-0.0 + -0.0) / 2.0
    assert M.cluster_one(S, 0.0)[1] == 1                 # v <= -0.0 holds for both zeros
    assert M.cluster_one(S, np.float32(1e-30))[1] == 3


def test_asymmetric_block_is_symmetrised_not_half_read():
    """the upper triangle alone would merge (0, 1) first, the lower alone (1, 2); the mean of the two merges (0, 2)"""
    S = np.array([[0, 5, 4], [-9, 0, 0], [4, 6, 0]], np.float32)
    up, lo = np.triu(S, 1), np.tril(S, -1)
    assert M.cluster_one((up + up.T).astype(np.float32), None, 2)[0].tolist() == [0, 0, 1]
    assert M.cluster_one((lo + lo.T).astype(np.float32), None, 2)[0].tolist() == [0, 1, 1]
    labels, k, ma, mb, mc = M.cluster_one(S, None, 2)
    assert labels.tolist() == [0, 1, 0] and mc[0] == -4.0


def test_non_finite_scores_are_counted_and_the_diagonal_is_ignored():
    S = M.gaussian(5, 1)
    S[2, 2] = np.nan
    M.cluster_one(S)
    S[1, 3] = np.nan
    S[4, 0] = np.inf
    with pytest.raises(M.NonFinite) as e:
        M.cluster_one(S)
    assert e.value.count == 2


def _blocks():
    return [M.gaussian(9, 1), M.integers(12, 2), M.gaussian(1, 3), M.all_equal(4), M.gaussian(20, 4), M.signed_zeros(6, 5)]


@pytest.mark.parametrize("threshold,num_speakers", [(0.3, None), (-0.2, None), (None, 1), (None, 3), (None, [1, 2, 1, 4, 5, 6]),
                                                    (0.1, 2), (-1.0, [3, 1, 1, 2, 9, 1]), (9.0, None)])
def test_cut_equals_a_run_with_the_same_arguments(threshold, num_speakers):
    from plda_amd import diarize
    blocks = _blocks()
    offsets = diarize.offsets_of([b.shape[0] for b in blocks])
    full = M.cluster(blocks, None, 1)
    labels, ncl = diarize.cut(full[2:], offsets, threshold, num_speakers)
    want = M.cluster(blocks, threshold, num_speakers)
    assert np.array_equal(labels, want[0]) and np.array_equal(ncl, want[1])
    assert labels.dtype == np.int32 and ncl.dtype == np.int32


def test_cut_refuses_a_partial_record_and_missing_stop_rule():
    from plda_amd import diarize
    blocks = _blocks()
    offsets = diarize.offsets_of([b.shape[0] for b in blocks])
    partial = M.cluster(blocks, 0.5, None)
    with pytest.raises(ValueError, match="not a full record"):
        diarize.cut(partial[2:], offsets, None, 1)
    with pytest.raises(ValueError, match="num_speakers"):
        diarize.cut(partial[2:], offsets, None, None)


def test_pack_and_merge_slices():
    from plda_amd import diarize
    blocks = _blocks()
    scores, block_off, offsets = diarize.pack(blocks)
    assert scores.dtype == np.float32 and block_off.tolist() == np.cumsum([0] + [b.size for b in blocks]).tolist()
    assert offsets.tolist() == np.cumsum([0] + [b.shape[0] for b in blocks]).tolist()
    sl = diarize.merge_slices(offsets)
    assert sl[0] == (0, 8) and sl[2] == (19, 19) and sl[-1][1] == int(offsets[-1]) - len(blocks)
    with pytest.raises(ValueError, match="square"):
        diarize.pack([np.zeros((2, 3), np.float32)])


def test_ctypes_signatures_exist():
    from plda_amd import _native as N
    import ctypes as C
    for name, nargs in (("plda_ahc_plan", 3), ("plda_ahc_matrix_dev", 13), ("plda_ahc_matrix", 13), ("plda_score_ahc_dev", 12),
                        ("plda_score_ahc", 12)):
        res, args = N.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
        assert hasattr(N.load(), name)
    assert N.SIGNATURES["plda_ahc_matrix"][1][5:7] == [C.c_int32, C.c_double]
    import plda_amd
    from liblda.plda import PLDA
    assert plda_amd.diarize.AHC_MAX == 4096 and hasattr(plda_amd.MPlda, "cluster") and hasattr(PLDA, "cluster")
