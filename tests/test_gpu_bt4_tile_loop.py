"""The tile loop of the one-wave-per-SIMD trials GEMM (plda_amd/csrc/score_bt4.inc) when ONE workgroup takes
several tiles in a row.

The code between two tiles of a workgroup -- the carried stores of the last block pair under the next tile's bias
MFMAs, the bias fragments read one tile ahead, the next tile's output base computed under the block-major part, the
straight-line advance of the DMA cursor, the rotation of the three bias slots, the queue table in front of the tile
table -- only runs when a workgroup's run of tiles is long.  The bit-identity shapes of test_gpu_bigtile.py give a
workgroup one or two tiles (at most 240 and 357 tiles on 256 workgroups).  Here every launch is ONE grid of >= 1 089
tiles (device-resident operands through score_matrix_dev: the host-pointer path cuts the matrix into slabs of 64 MiB
of scores), so every workgroup runs four tiles or more, its queue runs dry and it goes on in the next XCD's:

  * D = 200 (25 steps: 3,3,3,4,4,4,4), 8448 x 10240: 33 x 40 = 1 320 whole tiles;
  * D = 200, 8300 x 10100: the same grid with a fringe row and a fringe column -- fringe tiles inside a workgroup's run;
  * D = 72 (9 steps: 3,3,3 -- three stages, the smallest depth the kernel takes, where the precondition of the
    straight-line cursor advance is tight) and D = 96 (12 steps: 4,4,4), 8448 x 8448;
  * D = 56, 8448 x 8448: below the kernel's K = 72 -- PLDA_GEMM_VARIANT=40 must leave it to the kernel the dispatch
    picks there, and that one must agree as well.

Each with uniform and mixed enrol counts (the bucketed form: depth D + 4) as in
test_one_wave_per_simd_kernel_bit_identical.  The 256 x 256 kernel (PLDA_GEMM_VARIANT=40) and the 128 x 128 kernel
(=20) start every trial from the same bias value and contract in the same k order: np.array_equal over EVERY element.
The reference side is checked on its own against the per-trial C oracle (a 64 x 64 sample within score_tol), so that
a failure names the side that moved.
"""
import numpy as np
import pytest

from conftest import score_tol

pytestmark = pytest.mark.gpu

# (d, m, nt, the kernel variant 40 must run)
CASES = [(200, 8448, 10240, "bt4"), (200, 8300, 10100, "bt4"), (72, 8448, 8448, "bt4"), (96, 8448, 8448, "bt4"),
         (56, 8448, 8448, None)]


def _model(d, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    T = q * (1.0 + rng.random(d))[:, None]
    psi = np.sort(rng.random(d) * 4.0 + 0.05)[::-1].copy()
    return rng.random(d), T, psi


def _inputs(d, m, nt):
    rng = np.random.default_rng(1000 + d + m + nt)
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    counts = rng.integers(1, 6, m).astype(np.int32)
    return U, V, counts


def _scores(monkeypatch, variant, d, U, V, counts):
    """(uniform n = 2, mixed counts) of one launch each on device-resident operands, and the kernels that ran."""
    import torch
    from plda_amd import MPlda
    dev = torch.device("cuda", 0)
    monkeypatch.setenv("PLDA_GEMM_VARIANT", str(variant))
    eng = MPlda(0)
    mean, T, psi = _model(d, 3)
    eng.set_model(mean, T, psi)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    m, nt = U.shape[0], V.shape[0]
    dU, dV, dn = torch.from_numpy(U).to(dev), torch.from_numpy(V).to(dev), torch.from_numpy(counts).to(dev)
    outs, kernels = [], []
    for uniform in (True, False):
        out = torch.full((m, nt), float("nan"), dtype=torch.float32, device=dev)
        eng.score_matrix_dev(dU.data_ptr(), None if uniform else dn.data_ptr(), 2 if uniform else 0, m, dV.data_ptr(), nt,
                             out.data_ptr(), nt)
        torch.cuda.synchronize()
        kernels.append(eng.score_last_kernel())
        outs.append(out.cpu().numpy())
        del out
    eng.set_stream(None)
    return outs, kernels, psi


@pytest.mark.parametrize("d,m,nt,kernel40", CASES)
def test_long_tile_runs_bit_identical(monkeypatch, d, m, nt, kernel40):
    U, V, counts = _inputs(d, m, nt)
    ref, k20, _ = _scores(monkeypatch, 20, d, U, V, counts)
    got, k40, _ = _scores(monkeypatch, 40, d, U, V, counts)
    print("d=%d %dx%d: variant 20 ran %s, variant 40 ran %s" % (d, m, nt, k20, k40))
    for name in k20:
        assert "bt4" not in name and "bt2" not in name, k20
    for name in k40:
        if kernel40 is None:
            assert "bt4" not in name, k40          # K < 72: the dispatch must not hand this depth to the kernel
        else:
            assert kernel40 in name, k40
    for what, a, b in zip(("uniform", "mixed"), got, ref):
        assert a.shape == (m, nt) and b.shape == (m, nt)
        assert np.isfinite(b).all(), what
        assert np.isfinite(a).all(), what
        diff = a != b
        nbad = int(diff.sum())
        if nbad:
            rows, cols = np.nonzero(diff)
            print("%s: %d of %d elements differ; tiles (row, col) touched: %s" % (
                what, nbad, a.size, sorted(set(zip((rows >> 8).tolist(), (cols >> 8).tolist())))[:16]))
        assert np.array_equal(a, b), (d, m, nt, what, nbad)


@pytest.mark.parametrize("d,m,nt,kernel40", CASES)
def test_reference_side_against_oracle(monkeypatch, oracle, d, m, nt, kernel40):
    """The 128 x 128 kernel the comparison above leans on, against the per-trial fp64 oracle on a 64 x 64 sample (the
    matrix corners and the fringe included)."""
    U, V, counts = _inputs(d, m, nt)
    ref, _, psi = _scores(monkeypatch, 20, d, U, V, counts)
    rng = np.random.default_rng(d + nt)
    rows = np.unique(np.concatenate([[0, m - 1], rng.integers(0, m, 64)]))[:64]
    cols = np.unique(np.concatenate([[0, nt - 1], rng.integers(0, nt, 64)]))[:64]
    rows[-1], cols[-1] = m - 1, nt - 1
    for what, n, got in (("uniform", 2, ref[0]), ("mixed", counts[rows], ref[1])):
        want = oracle.score_block(psi, U[rows], n, V[cols])
        err = np.abs(got[np.ix_(rows, cols)].astype(np.float64) - want)
        print("%s: max |err| = %.3g (tolerance >= %.3g)" % (what, err.max(), score_tol(want).min()))
        assert (err <= score_tol(want)).all(), (what, err.max())
