"""CPU: the NumPy model of the spectral clustering (tests/spectral_model.py) against independent restatements and hand-written
cases.  The GPU tests (tests/test_gpu_spectral.py) hold the device to this model."""
import numpy as np
import pytest

import spectral_model as M


@pytest.mark.parametrize("n,levels,p", [(9, 2, 3), (17, 3, 5), (40, 4, 39), (33, 8, 1), (25, 1, 7)])
def test_neighbours_against_stable_argsort(n, levels, p):
    """rows with many equal scores: the sort-by-key selection and the stable argsort agree, and ties go to the lower j"""
    c = M.similarity(M.quantised(n, levels, 100 * n + p))
    c[c == 0] = -0.0                                        # (signed zeros are one value)
    c[::2, 1::2] = np.abs(c[::2, 1::2])
    c = (c + c.T) / 2.0
    B = M.neighbours(c, p)
    assert np.array_equal(B, M.neighbours_fast(c, p))
    pe = min(p, n - 1)
    assert (B.sum(1) == pe).all() and (np.diag(B) == 0).all()
    for i in range(n):
        kept = np.flatnonzero(B[i])
        worst = c[i, kept].min()
        for j in range(n):
            if j != i and not B[i, j]:
                assert c[i, j] < worst or (c[i, j] == worst and j > kept[c[i, kept] == worst].max())


def test_equal_scores_keep_the_lowest_indices():
    B = M.neighbours(M.similarity(M.all_equal(6)), 2)
    assert np.array_equal(np.flatnonzero(B[0]), [1, 2]) and np.array_equal(np.flatnonzero(B[1]), [0, 2])
    assert np.array_equal(np.flatnonzero(B[5]), [0, 1])


def test_n1_n2_n3_by_hand():
    r = M.spectral(np.zeros((1, 1), np.float32), [3, 1], max_speakers=4)
    assert r["labels"].tolist() == [0] and r["n_clusters"] == 1 and r["p_used"] == 0 and r["k_gap"] == 1
    assert r["eig"].shape == (2, 6) and r["eig"][0, 0] == 0 and r["eig"][0, -1] == 0 and np.isinf(r["eig"][:, 1:-1]).all()
    # N = 2: one edge, L = [[1, -1], [-1, 1]], eigenvalues 0 and 2, one gap: k_gap = 1 -> one cluster
    r = M.spectral(np.array([[9, 0.5], [0.25, 9]], np.float32), [5], max_speakers=4)
    assert np.array_equal(r["L"], [[1, -1], [-1, 1]]) and r["deg2"].tolist() == [2, 2]
    assert np.allclose(r["eig"][0, :2], [0, 2], atol=1e-15) and np.isinf(r["eig"][0, 2:-1]).all() and abs(r["eig"][0, -1] - 2) < 1e-15
    assert r["p_used"] == 1 and r["k_gap"] == 1 and r["labels"].tolist() == [0, 0] and r["n_clusters"] == 1
    assert abs(r["rs"][0] - 1.0 / (2.0 / (2.0 + 1e-10))) < 1e-15
    # ... and two clusters when the count is given: the second column separates the two rows
    r = M.spectral(np.array([[9, 0.5], [0.25, 9]], np.float32), [5], max_speakers=4, num_speakers=2)
    assert r["labels"].tolist() == [0, 1] and r["n_clusters"] == 2
    # N = 3, p = 1: 0 and 1 choose each other, 2 chooses 0 (c(2, 0) = 0.3 > c(2, 1) = 0.1): a path 1 - 0 - 2 with weights 1, 1/2
    S = np.array([[0, 0.9, 0.3], [0.9, 0, 0.1], [0.3, 0.1, 0]], np.float32)
    r = M.spectral(S, [1], max_speakers=4)
    assert np.array_equal(r["L"], [[1.5, -1, -0.5], [-1, 1, 0], [-0.5, 0, 0.5]]) and r["deg2"].tolist() == [3, 2, 1]
    lam = np.linalg.eigvalsh(r["L"])                        # 0, (3 - sqrt 3) / 2, (3 + sqrt 3) / 2
    assert np.allclose(lam, [0, (3 - np.sqrt(3)) / 2, (3 + np.sqrt(3)) / 2], atol=1e-14)
    assert r["k_gap"] == 2 and r["n_clusters"] == 2 and r["labels"].tolist() == [0, 0, 1]


def test_sweep_ties_and_forced_count():
    eig = np.array([[0, 1, 3, np.inf, 4.0], [0, 1, 3, np.inf, 4.0], [0, 0.5, 3.5, np.inf, 4.0]])
    pos, p_used, k_gap, rs = M.choose(eig, 3, [2, 2, 1], 3)
    assert rs[0] == rs[1] and pos == 2 and p_used == 1 and k_gap == 2        # r = 1 / (3 / 4) beats 2 / (2 / 4)
    pos, p_used, _, _ = M.choose(eig[:2], 3, [9, 2], 3)
    assert pos == 0 and p_used == 2                                          # equal p_eff and r: the earlier position
    flat = np.array([[1.0, 1.0, np.inf, np.inf, 1.0]])
    assert M.choose(flat, 2, [1], 3)[3] == [np.inf]                          # g <= 0: r = +inf, still chosen


@pytest.mark.parametrize("n,k", [(24, 2), (60, 3), (100, 4), (161, 5)])
def test_planted_partitions_recovered(n, k):
    S, lab = M.planted(n, k, 0.1, 5 * n + k)
    r = M.spectral(S, M.default_p(n), max_speakers=8)
    assert r["n_clusters"] == k and M.same_partition(r["labels"], lab)
    assert r["labels"][0] == 0 and (np.diff(np.unique(r["labels"])) == 1).all()


def test_kmeans_invariant_under_change_of_basis():
    """the labels do not depend on the basis the eigensolver returns: a random orthogonal change of basis of U plus noise at
    1e-11 leaves them unchanged on planted blocks (60 seeds)"""
    differ = 0
    for seed in range(60):
        n, k = 20 + 3 * seed, 2 + seed % 4
        S, _ = M.planted(n, k, 0.4, 1000 + seed)
        r = M.spectral(S, M.default_p(n)[:3], max_speakers=8)
        kk = r["k"]
        U = r["embed"][:, :kk]
        rng = np.random.default_rng(seed)
        Q, _ = np.linalg.qr(rng.standard_normal((kk, kk)))
        lab2, ncl2 = M.kmeans(U @ Q + 1e-11 * rng.standard_normal(U.shape))
        differ += int(ncl2 != r["n_clusters"] or not np.array_equal(lab2, r["labels"]))
    assert differ == 0


def test_kmeans_empty_centre_and_iteration_cap():
    U = np.array([[0.0], [0.0], [0.0]])
    lab, ncl = M.kmeans(np.hstack([U, U]))                  # k = 2 on three equal rows: centre 1 = row 0 again, stays empty
    assert lab.tolist() == [0, 0, 0] and ncl == 1
    # centres 0 and 19; step 1 sends 10 to 19 (10 against 9) and the centres move to 16 / 3 and 46 / 3; step 2 brings it back
    # (4.67 against 5.33); step 3 moves nothing
    x = np.array([[0.0, 0], [8, 0], [8, 0], [10, 0], [17, 0], [19, 0]])
    one, _ = M.kmeans(x, max_iters=1)
    full, _ = M.kmeans(x, max_iters=20)
    assert one.tolist() == [0, 0, 0, 1, 1, 1] and full.tolist() == [0, 0, 0, 0, 1, 1]
    assert M.kmeans(x, max_iters=2)[0].tolist() == full.tolist()
