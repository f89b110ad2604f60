"""The classical hard inputs of a divide-and-conquer symmetric eigensolver, shared by tests/test_gpu_eig.py (the device
kernels of csrc/eig_dc.hip) and tests/test_proto_dc_eig.py (their NumPy prototype, whose `stats` show that the cases
really produce the merges they are for).  Random and random-orthogonal-basis matrices only ever give a merge every
pole (k = n) or none (total deflation); these give merges with one or two surviving poles, long runs of type-2
deflation (equal eigenvalues rotated into each other one by one), negative off-diagonals (the sign of the tear) and
close-but-coupled eigenvalues, where such solvers lose orthogonality.

Tridiagonal cases are returned as dense tridiagonal matrices: the Householder step finds every column already
tridiagonal and passes d, e through unchanged (up to its power-of-two scaling), so the divide and conquer sees exactly
the matrix written here, torn at row n // 2 and below."""
import numpy as np

EPS = np.finfo(np.float64).eps


def tridiag(d, e):
    d, e = np.asarray(d, np.float64), np.asarray(e, np.float64)
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def wilkinson_diag(m):
    """diagonal of W+ of odd order m: |i - (m - 1) / 2|, off-diagonals 1."""
    return np.abs(np.arange(m) - (m - 1) // 2).astype(np.float64)


def wilkinson(n):
    """W+ of the largest odd order <= n; an even n gets one decoupled trailing entry."""
    m = n if n % 2 else max(n - 1, 1)
    d = np.concatenate([wilkinson_diag(m), np.full(n - m, 0.5)])
    e = np.ones(n - 1)
    e[m - 1:] = 0.0
    return tridiag(d, e)


def glued_wilkinson(n, block, delta):
    """copies of W+_block along the diagonal (the last one cut off at n), off-diagonal delta at the joins."""
    d = np.resize(wilkinson_diag(block), n)
    e = np.ones(n - 1)
    e[block - 1::block] = delta
    return tridiag(d, e)


def middle_coupling(d, c):
    e = np.zeros(len(d) - 1)
    if len(e):
        e[max(len(d) // 2 - 1, 0)] = c      # the off-diagonal the top-level tear removes
    return tridiag(d, e)


def hard_cases(n, rng):
    """[(name, symmetric n x n matrix)]; the list has the same length and order for every n."""
    i = np.arange(n)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ones_twos = np.concatenate([np.ones(n // 2), np.full(n - n // 2, 2.0)])
    out = [
        ("wilkinson", wilkinson(n)),
        ("glued wilkinson 21 1e-4", glued_wilkinson(n, 21, 1e-4)),
        ("glued wilkinson 15 1e-8", glued_wilkinson(n, 15, 1e-8)),
        ("glued wilkinson 21 1e-14", glued_wilkinson(n, 21, 1e-14)),
        ("toeplitz 1-2-1 negative", tridiag(np.full(n, 2.0), np.full(n - 1, -1.0))),
        ("clement", tridiag(np.zeros(n), np.sqrt((i[:-1] + 1.0) * (n - 1.0 - i[:-1])))),
        ("alternating signs", tridiag(rng.standard_normal(n), (0.5 + rng.random(n - 1)) * (-1.0) ** i[:-1])),
        ("graded couplings", tridiag(rng.standard_normal(n), 10.0 ** -rng.integers(0, 17, n - 1).astype(np.float64))),
        ("identity one coupling", middle_coupling(np.ones(n), 0.25)),
        ("ones twos one coupling", middle_coupling(ones_twos, 0.25)),
        ("ones twos tiny coupling", middle_coupling(ones_twos, 1e-13)),
        ("dense 1 + 4 eps i", (q * (1.0 + 4.0 * EPS * i)) @ q.T),
        ("dense one large rest 1e-14", (q * np.concatenate([[1.0], np.full(n - 1, 1e-14)])) @ q.T),
    ]
    return [(name, 0.5 * (G + G.T)) for name, G in out]


N_HARD = 13
