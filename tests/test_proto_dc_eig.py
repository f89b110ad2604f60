"""CPU: the NumPy prototype of the device eigensolver (scripts/proto_dc_eig.py: Householder tridiagonalisation +
divide and conquer with dlaed2-style deflation, two-pole secular iteration, Gu-Eisenstat vectors) against
numpy.linalg.eigh on the hard cases.  csrc/eig_dc.hip implements the same rules (tests/test_gpu_eig.py checks the
kernels); this keeps the restatement they were developed against honest."""
import importlib.util
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location(
    "proto_dc_eig", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "proto_dc_eig.py"))
proto = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(proto)


def _cases(n, rng):
    A = rng.standard_normal((n, n))
    yield "gaussian", A + A.T
    B = rng.standard_normal((n, max(n // 3, 1)))
    yield "rank-deficient", B @ B.T
    yield "identity", np.eye(n)
    yield "zero", np.zeros((n, n))
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    yield "two clusters", (q * np.concatenate([np.ones(n // 2), np.full(n - n // 2, 2.0)])) @ q.T
    yield "graded", (q * 10.0 ** (-np.arange(n) * 16.0 / n)) @ q.T
    yield "scaled 1e-150", (A + A.T) * 1e-150


@pytest.mark.parametrize("n", [1, 2, 5, 17, 33, 64, 100])
def test_prototype_matches_numpy(n):
    rng = np.random.default_rng(n)
    for name, G in _cases(n, rng):
        G = 0.5 * (G + G.T)
        lam, Z = proto.sym_eig(G)
        ref = np.linalg.eigvalsh(G)[::-1]
        nrm = max(np.abs(ref).max(), 1e-300)
        assert np.abs(lam - ref).max() / nrm < 1e-13, (name, n)
        assert np.abs(Z.T @ Z - np.eye(n)).max() < 1e-12, (name, n)
        assert np.abs(G @ Z - Z * lam[None, :]).max() / nrm < 1e-12, (name, n)


def test_secular_roots_interlace():
    """roots of 1 + rho sum z_i^2 / (d_i - lam): exactly one in each (d_j, d_j+1), the last in (d_k, d_k + rho |z|^2]."""
    rng = np.random.default_rng(3)
    d = np.sort(rng.random(40)) ; z = rng.standard_normal(40) ; z /= np.linalg.norm(z)
    org, mu, delta = proto.secular_roots(d, z, 0.7)
    lam = d[org] + mu
    assert (lam[:-1] > d[:-1]).all() and (lam[:-1] < d[1:]).all() and d[-1] < lam[-1] <= d[-1] + 0.7 + 1e-15
    ref = np.linalg.eigvalsh(np.diag(d) + 0.7 * np.outer(z, z))
    assert np.abs(lam - ref).max() < 1e-14


import eig_hard_cases as hc


def _run_hard(name, G):
    n = G.shape[0]
    st = []
    lam, Z = proto.sym_eig(G, stats=st)
    ref = np.linalg.eigvalsh(G)[::-1]
    nrm = max(np.abs(ref).max(), 1e-300)
    e_val = np.abs(lam - ref).max() / nrm
    e_orth = np.abs(Z.T @ Z - np.eye(n)).max()
    e_res = np.abs(G @ Z - Z * lam[None, :]).max() / nrm
    assert e_val < 1e-13 and e_orth < 1e-12 and e_res < 1e-12, (name, n, e_val, e_orth, e_res)
    return st, (e_val, e_orth, e_res)


@pytest.mark.parametrize("n", [21, 33, 101, 105, 210])
def test_prototype_on_the_hard_cases(n):
    """The classical hard inputs of divide and conquer (tests/eig_hard_cases.py) at the prototype's own bounds (measured
    worst over all of them: 4.3e-15 / 3.1e-15 / 1.8e-15), and -- through `stats`, one (size, surviving poles k) per merge
    that reaches the secular equation, the top level last -- that each case produces the merge it is for.  The device
    applies the same deflation rule, so this keeps the GPU cases of tests/test_gpu_eig.py honest if the rule changes."""
    cases = dict(hc.hard_cases(n, np.random.default_rng(n)))
    assert len(cases) == hc.N_HARD
    stats = {}
    for name, G in cases.items():
        stats[name], _ = _run_hard(name, G)
    # identity + one coupling at the tear: both halves are diagonal (their merges find nothing coupled and record
    # nothing), the top-level z has two equal poles, one rotates into the other: exactly one merge, k = 1
    assert stats["identity one coupling"] == [(n, 1)]
    # two distinct eigenvalues on either side of the tear, with an O(1) and with a tiny rho
    assert stats["ones twos one coupling"][-1] == (n, 2)
    assert stats["ones twos tiny coupling"][-1] == (n, 2)
    # Toeplitz of even order: the torn halves are mirror images, every pole of one meets its equal in the other and
    # rotates into it: half of them deflate (an odd order has halves of different size and keeps every pole)
    assert stats["toeplitz 1-2-1 negative"][-1] == ((n, n // 2) if n % 2 == 0 else (n, n))
    if n >= 105:
        # glued at 1e-14: whatever crosses a join deflates, a merge never keeps more poles than one copy has
        big = [(m, k) for m, k in stats["glued wilkinson 21 1e-14"] if m >= 105]
        assert big and all(k <= 21 for _, k in big), big
