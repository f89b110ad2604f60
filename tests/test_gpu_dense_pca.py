"""GPU: recording-dependent PCA before dense PLDA scoring (K19; csrc/dense_pca.hip) against the NumPy model of
tests/dense_pca_model.py.

Inputs have a planted spectrum (Gaussian rows times a geometric scale, ratio 0.7, times a random orthogonal matrix, plus an
offset).  Before comparing, every test asserts on the MODEL's own numbers that the cumulative energy share stays 1e-6 away from
the target at every k and that the cut is at least 1e-3 lam_1 wide, so that rounding cannot move the retained dimension.

Bounds: dims equal; eigenvalues within 1e-12 lam_1 (m eps <= 6e-14 at m = 512); every block within 2^-22 max|S_model| of the
model rounded to fp32 (one fp32 rounding plus an fp64 error far below it).  The ill-conditioned case has no fixed bound: the
device may deviate from the model's eigh route by 10 x the spread between the model's eigh and SVD routes (its cut lies below a
direction of 1e-6 lam_1, so the 1e-3 lam_1 gap cannot hold there; the test asserts a factor 2 between the last retained and
the first dropped eigenvalue instead)."""
import ctypes as C
import gc

import numpy as np
import pytest

import dense_pca_model as dm
from history_cases import dense_pca_case

pytestmark = pytest.mark.gpu

BLOCK_TOL = 2.0 ** -22
EIG_TOL = 1e-12


def _engine(model):
    from plda_amd import MPlda
    eng = MPlda(0)
    eng.set_model(model["mean"], model["transform"], model["psi"])
    return eng


def _assert_margins(x, offsets, target):
    for r in range(len(offsets) - 1):
        share, gap = dm.margins(dm.pca(x[offsets[r]:offsets[r + 1]])[0], target)
        assert share >= 1e-6, "recording %d: energy share within %g of the target" % (r, share)
        assert gap >= 1e-3, "recording %d: gap at the cut %g lam_1" % (r, gap)


def _parity(eng, model, x, offsets, target, margins=True):
    from plda_amd import diarize
    if margins:
        _assert_margins(x, offsets, target)
    ref, rdims, reig = dm.score_blocks(model, x, offsets, target)
    blocks, info = diarize.score_dense_pca(eng, x, offsets, target, return_info=True)
    assert np.array_equal(info["dims"], rdims), (info["dims"], rdims)
    for r, (got, want) in enumerate(zip(blocks, ref)):
        a, n = int(offsets[r]), int(offsets[r + 1] - offsets[r])
        m = min(n, x.shape[1])
        lam = reig[a:a + m]
        err = np.abs(info["eigenvalues"][r] - lam).max()
        assert err <= EIG_TOL * max(lam[0], np.finfo(float).tiny), "recording %d (N = %d): eigenvalues off by %g lam_1" % (r, n, err / lam[0])
        assert got.dtype == np.float32 and got.shape == (n, n)
        bound = BLOCK_TOL * np.abs(want).max()
        dev = np.abs(got.astype(np.float64) - want.astype(np.float32).astype(np.float64)).max()
        assert dev <= bound, "recording %d (N = %d, d = %d): block off by %g, bound %g" % (r, n, rdims[r], dev, bound)
    return blocks, info


# ------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("d,sizes", [(8, (1, 2, 3, 63, 64, 65)), (72, (1, 2, 3, 63, 64, 65, 300))])
def test_parity_small_shapes(d, sizes):
    """N <= D: the Gram route (odd m: the bye); N > D: the covariance route, N = 300 with the rows streamed."""
    model, x, offsets = dm.case(100 + d, sizes, d, 0.3)
    eng = _engine(model)
    _, info = _parity(eng, model, x, offsets, 0.3)
    assert info["dims"][0] == 0                      # N = 1: no variance
    t2 = 0.9 if d == 8 else 0.5
    model, x, offsets = dm.case(200 + d, sizes, d, t2)
    _parity(_engine(model), model, x, offsets, t2)


def test_lds_class_limit():
    """m at the LDS class's limit and one above it (the plan says which class each takes)."""
    from plda_amd import diarize
    d = 128
    model, _, _ = dm.case(7, (4,), d, 0.3, check=False)
    eng = _engine(model)
    lim = diarize.dense_pca_plan(eng, 1, d)["lds_max"]
    assert 8 <= lim < d
    p0, p1 = diarize.dense_pca_plan(eng, lim, d), diarize.dense_pca_plan(eng, lim + 1, d)
    assert (p0["cls"], p0["m"], p1["cls"], p1["m"]) == (0, lim, 1, lim + 1)
    assert p0["scratch_bytes"] > 0 and p1["scratch_bytes"] > p0["scratch_bytes"]
    assert diarize.dense_pca_plan(eng, 4000, d)["m"] == d
    model, x, offsets = dm.case(8, (lim, lim + 1, lim - 1), d, 0.5)
    _parity(_engine(model), model, x, offsets, 0.5)


def test_cap_dimension():
    """One recording at D = 512, N = 520: the largest eigenproblem, in the HBM class."""
    model, x, offsets = dm.case(9, (520,), 512, 0.5)
    _parity(_engine(model), model, x, offsets, 0.5)


def _raw(eng, x, offsets, target, block_off=None):
    from plda_amd import _native as N
    x = np.ascontiguousarray(x, np.float64)
    offsets = np.ascontiguousarray(offsets, np.int64)
    sizes = np.diff(offsets)
    if block_off is None:
        block_off = np.concatenate([[0], np.cumsum(np.abs(sizes) ** 2)]).astype(np.int64)
    scores = np.zeros(max(int(block_off[-1]), 1), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = eng._lib.plda_score_dense_pca(eng._h, p(x), p(offsets), len(offsets) - 1, float(target), p(scores), p(block_off), None, None)
    return rc, eng._lib.plda_last_error(eng._h).decode()


def test_rejected_arguments():
    from plda_amd import MPlda, diarize
    from plda_amd import _native as N
    rng = np.random.default_rng(3)
    # D = 513
    big = dm.random_model(rng, 513)
    eng = _engine(big)
    x = rng.standard_normal((6, 513))
    with pytest.raises(ValueError):
        diarize.score_dense_pca(eng, x, [0, 6], 0.3)
    assert _raw(eng, x, [0, 6], 0.3)[0] == N.PLDA_E_INVAL
    # a truncated model
    model = dm.random_model(rng, 8)
    eng = _engine({"mean": model["mean"], "transform": model["transform"][:5], "psi": model["psi"][:5]})
    x = rng.standard_normal((6, 8))
    with pytest.raises(ValueError):
        diarize.score_dense_pca(eng, x, [0, 6], 0.3)
    with pytest.raises(ValueError):
        eng.cluster(x, [0, 6], 0.0, target_energy=0.3)
    assert _raw(eng, x, [0, 6], 0.3)[0] == N.PLDA_E_INVAL
    # no model
    assert _raw(MPlda(0), x, [0, 6], 0.3)[0] == N.PLDA_E_NOT_FITTED
    # everything else the host can see
    eng = _engine(model)
    for t in (0.0, 1.0, -0.1, float("nan")):
        assert _raw(eng, x, [0, 6], t)[0] == N.PLDA_E_INVAL
        with pytest.raises(ValueError):
            diarize.score_dense_pca(eng, x, [0, 6], t)
    for off in ([1, 6], [0, 3, 3, 6], [0, 4, 2]):
        assert _raw(eng, x, off, 0.3)[0] == N.PLDA_E_INVAL
        with pytest.raises(ValueError):
            diarize.score_dense_pca(eng, x, off, 0.3)
    assert _raw(eng, np.zeros((4097, 8)), [0, 4097], 0.3, np.asarray([0, 1], np.int64))[0] == N.PLDA_E_INVAL   # above PLDA_AHC_MAX
    assert _raw(eng, x, [0, 2, 6], 0.3, np.asarray([0, 4, 19], np.int64))[0] == N.PLDA_E_INVAL     # 15 < 4 x 4
    # NaN rows: the count in the message (the Python wrapper sees them first)
    bad = x.copy()
    bad[1, 2] = np.nan
    bad[4, 0] = np.inf
    rc, msg = _raw(eng, bad, [0, 2, 6], 0.3)
    assert rc == N.PLDA_E_INVAL and "2 row" in msg, msg
    with pytest.raises(ValueError):
        diarize.score_dense_pca(eng, bad, [0, 2, 6], 0.3)
    assert _raw(eng, x, [0, 2, 6], 0.3)[0] == 0                                                    # and the handle still works


# ------------------------------------------------------------------------------------------------------------ batch
def test_batch_is_bit_equal_to_single_calls_and_to_other_groupings(monkeypatch):
    """40 recordings of 1 ... 150 segments at D = 128 (both dispatch classes) in one call; every block bit-equal to the same
    recording scored alone, and to a handle whose scratch budget forces several launch groups."""
    from plda_amd import diarize
    rng = np.random.default_rng(11)
    sizes = [1, 2, 150, 101, 100] + [int(v) for v in rng.integers(3, 151, 35)]
    model, x, offsets = dm.case(12, sizes, 128, 0.3)
    eng = _engine(model)
    blocks, info = _parity(eng, model, x, offsets, 0.3)
    for r in range(len(sizes)):
        xr = x[offsets[r]:offsets[r + 1]]
        (alone,), one = diarize.score_dense_pca(eng, xr, [0, len(xr)], 0.3, return_info=True)
        assert np.array_equal(alone.view(np.uint32), blocks[r].view(np.uint32)), "recording %d differs alone" % r
        assert one["dims"][0] == info["dims"][r]
        assert np.array_equal(one["eigenvalues"][0].view(np.uint64), info["eigenvalues"][r].view(np.uint64))
    monkeypatch.setenv("PLDA_AHC_SCRATCH_BYTES", str(3 << 20))
    small = _engine(model)
    monkeypatch.delenv("PLDA_AHC_SCRATCH_BYTES")
    per = [diarize.dense_pca_plan(small, n, 128)["scratch_bytes"] for n in sizes]
    assert sum(per) > 3 * (3 << 20)                  # several groups
    again = diarize.score_dense_pca(small, x, offsets, 0.3)
    for r in range(len(sizes)):
        assert np.array_equal(again[r].view(np.uint32), blocks[r].view(np.uint32)), "recording %d differs under another grouping" % r
    la, ka, ma = diarize.ahc_dense_pca(eng, x, offsets, 0.3, None, 1, True)
    lb, kb, mb = diarize.ahc_dense_pca(small, x, offsets, 0.3, None, 1, True)     # several slabs, several groups
    assert np.array_equal(la, lb) and np.array_equal(ka, kb)
    for a, b in zip(ma, mb):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("threshold", [None, 0.0])
def test_ahc_form_over_three_slabs_equals_single_calls(monkeypatch, threshold):
    """plda_score_dense_pca_ahc when the blocks take three slabs: recordings of 3, 70, 1, 200 and 9 segments are 64 + 4928 + 64,
    40000 and 128 padded floats, and a budget of 5056 floats holds the first three exactly, then the fourth alone (it is larger
    than the budget), then the fifth.  With min_clusters per recording and the merge record asked for, every recording's labels,
    count and entries of the record equal the same recording's in a call of its own: the slabs' outputs start at offsets[r0],
    r0 and offsets[r0] - r0 of the caller's arrays, and min_clusters is read from r0 on."""
    from plda_amd import diarize
    sizes, minc = [3, 70, 1, 200, 9], [2, 3, 1, 4, 2]
    padded = [(n * n + 63) // 64 * 64 for n in sizes]
    assert padded[0] + padded[1] + padded[2] == 5056 and padded[3] > 5056
    model, x, offsets = dm.case(19, sizes, 32, 0.3)
    monkeypatch.setenv("PLDA_AHC_SCRATCH_BYTES", str(4 * 5056))
    small = _engine(model)
    monkeypatch.delenv("PLDA_AHC_SCRATCH_BYTES")
    eng = _engine(model)
    labels, ncl, merges = diarize.ahc_dense_pca(small, x, offsets, 0.3, threshold, minc, True)
    for r, (m0, m1) in enumerate(diarize.merge_slices(offsets)):
        xr = x[offsets[r]:offsets[r + 1]]
        l1, k1, g1 = diarize.ahc_dense_pca(eng, xr, [0, len(xr)], 0.3, threshold, minc[r], True)
        assert np.array_equal(labels[offsets[r]:offsets[r + 1]], l1) and ncl[r] == k1[0], "recording %d" % r
        assert k1[0] >= minc[r] and (threshold is not None or k1[0] == minc[r])
        for a, b in zip(merges, g1):
            assert np.array_equal(a[m0:m1], b), "recording %d: merge record" % r


# ------------------------------------------------------------------------------------- facts independent of the model
def test_full_dimension_equals_the_full_model():
    """target 0.9999 and N > D: the model keeps every direction, and the scores are the full model's (oracle LLR)."""
    from oracle import plda_oracle_np as onp
    from plda_amd import diarize
    d = 8
    model, x, offsets = dm.case(21, (40, 30), d, 0.9999)
    _, rdims, _ = dm.score_blocks(model, x, offsets, 0.9999)
    assert (rdims == d).all()
    full = dict(model, offset=-model["transform"] @ model["mean"])
    blocks, info = diarize.score_dense_pca(_engine(model), x, offsets, 0.9999, return_info=True)
    assert (info["dims"] == d).all()
    for r, got in enumerate(blocks):
        y = onp.transform_ivector(full, x[offsets[r]:offsets[r + 1]], 1)
        want = onp.llr_matrix(model["psi"], y, 1, y)
        assert np.abs(got - want.astype(np.float32)).max() <= BLOCK_TOL * np.abs(want).max()


def test_equal_rows_give_a_zero_block_and_one_cluster():
    from plda_amd import diarize
    rng = np.random.default_rng(5)
    model = dm.random_model(rng, 8)
    eng = _engine(model)
    x = np.tile(rng.standard_normal(8), (7, 1))
    (blk,), info = diarize.score_dense_pca(eng, x, [0, 7], 0.3, return_info=True)
    assert info["dims"][0] == 0
    assert np.array_equal(blk.view(np.uint32), np.zeros((7, 7), np.uint32))          # +0.0f, bit for bit
    labels, ncl = eng.cluster(x, [0, 7], threshold=0, target_energy=0.3)
    assert ncl[0] == 1 and (labels == 0).all()


def test_ill_conditioned_spectrum():
    """A planted spectrum spanning 1e-6, target 0.99999: directions near 1e-6 lam_1 are retained.  The device may deviate from
    the model's eigh route by 10 x the spread between the model's eigh and SVD routes (both backward stable)."""
    from plda_amd import diarize
    model, x, offsets, target = dm.ill_conditioned_case()
    lam = dm.pca(x)[0]
    share, _ = dm.margins(lam, target)
    d = dm.retained(lam, target)
    assert share >= 1e-6 and d >= 2 and lam[d - 1] <= 1e-5 * lam[0]
    assert d == len(lam) or lam[d - 1] >= 2.0 * lam[d]
    s_eigh, d1, _ = dm.score_block(model, x, target, "eigh")
    s_svd, d2, _ = dm.score_block(model, x, target, "svd")
    assert d1 == d2 == d
    spread = np.abs(s_eigh - s_svd).max()
    (blk,), info = diarize.score_dense_pca(_engine(model), x, offsets, target, return_info=True)
    assert info["dims"][0] == d
    assert np.abs(info["eigenvalues"][0] - lam).max() <= EIG_TOL * lam[0]
    dev = np.abs(blk.astype(np.float64) - s_eigh).max()
    rounding = 2.0 ** -24 * np.abs(s_eigh).max()                 # the one fp32 rounding of the device's block
    print("ill-conditioned: eigh/svd spread %g, device deviation %g (fp32 rounding %g)" % (spread, dev, rounding))
    assert dev <= 10.0 * spread + rounding


# ------------------------------------------------------------------------------------------------------------ chain
def test_chain_cluster_tune_and_untouched_default():
    from plda_amd import der, diarize
    rng = np.random.default_rng(31)
    sizes = [30, 7, 120, 64, 1, 2]
    model, x, offsets = dm.case(32, sizes, 24, 0.3)
    eng = _engine(model)
    t = 0.3
    blocks = diarize.score_dense_pca(eng, x, offsets, t)
    for thr, spk in ((0.0, None), (None, 2), (1.5, 3)):
        want = diarize.ahc(eng, blocks, thr, spk, True)
        got = diarize.ahc_dense_pca(eng, x, offsets, t, thr, spk, True)
        viam = eng.cluster(x, offsets, thr, spk, True, target_energy=t)
        for res in (got, viam):
            assert np.array_equal(res[0], want[0]) and np.array_equal(res[1], want[1])
            for a, b in zip(res[2], want[2]):
                assert np.array_equal(a, b)
    # target_energy=None is today's path, bit for bit
    a = eng.cluster(x, offsets, 0.0, None, True)
    b = eng.cluster(x, offsets, 0.0, None, True, target_energy=None)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for u, v in zip(a[2], b[2]):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    # tune_threshold(target_energy=t) = a manual sweep over the same record
    ref = np.concatenate([rng.integers(0, 3, n) for n in sizes]).astype(np.int32)
    thresholds = np.linspace(-3.0, 3.0, 7)
    best, res = eng.tune_threshold(x, offsets, ref, thresholds, target_energy=t)
    _, _, merges = eng.cluster(x, offsets, None, 1, True, target_energy=t)
    manual = der.sweep(eng, merges, offsets, ref, thresholds, None)
    assert best == float(manual.thresholds[manual.best])
    assert np.array_equal(res.counts, manual.counts) and np.array_equal(res.n_clusters, manual.n_clusters)
    # diarize: the PCA goes to the clustering only
    lab, _ = eng.cluster(x, offsets, 0.0, None, target_energy=t)
    want = eng.resegment(x, offsets, lab)
    got = eng.diarize(x, offsets, 0.0, None, target_energy=t)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_model_change_drops_the_cached_covariances():
    """W and B are formed once per model and kept on the handle: a second call reuses them bit for bit, a new model of the same
    dimension replaces them."""
    from plda_amd import diarize
    m1, x, offsets = dm.case(71, (30, 9), 16, 0.5)
    m2 = dm.random_model(np.random.default_rng(72), 16)
    eng = _engine(m1)
    first = _parity(eng, m1, x, offsets, 0.5)[0]
    again = diarize.score_dense_pca(eng, x, offsets, 0.5)
    eng.set_model(m2["mean"], m2["transform"], m2["psi"])
    other = _parity(eng, m2, x, offsets, 0.5)[0]
    fresh = diarize.score_dense_pca(_engine(m2), x, offsets, 0.5)
    for r in range(2):
        assert np.array_equal(first[r].view(np.uint32), again[r].view(np.uint32))
        assert np.array_equal(other[r].view(np.uint32), fresh[r].view(np.uint32))
        assert not np.array_equal(first[r], other[r])


# ------------------------------------------------------------------------------------------------------- robustness
def test_poisoned_scratch_is_bit_identical(monkeypatch):
    from plda_amd import MPlda, diarize
    sizes = [5, 101, 64, 1, 130, 33]
    model, x, offsets = dm.case(41, sizes, 110, 0.5)
    out = {}
    for poison in (False, True):
        if poison:
            monkeypatch.setenv("PLDA_SCRATCH_POISON", "1")
        else:
            monkeypatch.delenv("PLDA_SCRATCH_POISON", raising=False)
        eng = _engine(model)
        monkeypatch.delenv("PLDA_SCRATCH_POISON", raising=False)
        out[poison] = list(dense_pca_case(x, offsets, 0.5)(eng).values())       # (shared with tests/test_gpu_handle_history.py)
        eng.synchronize()
        del eng
    MPlda(0)                                         # the switch off again for whatever runs next in this process
    for a, b in zip(out[False], out[True]):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    _parity(_engine(model), model, x, offsets, 0.5)


def test_guard_bands_stay_untouched():
    """dscores, ddims and deig inside buffers filled with a payload, X between NaN neighbours: no store outside the outputs,
    no block element left unwritten, and the same bits as the host form."""
    import torch
    from plda_amd import diarize
    dev = torch.device("cuda", 0)
    payload, g = 0x7FC0DEAD, (64 << 10) // 4
    sizes = [9, 101, 2, 40]
    model, x, offsets = dm.case(51, sizes, 104, 0.5)
    eng = _engine(model)
    t_rows, r = int(offsets[-1]), len(sizes)
    gap = 13                                         # floats of slack between blocks: guards between them as well
    block_off = np.zeros(r + 1, np.int64)
    for q, n in enumerate(sizes):
        block_off[q + 1] = block_off[q] + n * n + gap
    xin = torch.full((g + x.size + g,), float("nan"), dtype=torch.float64, device=dev)
    xin[g:g + x.size] = torch.from_numpy(x.ravel()).to(dev)
    ws = torch.full((g + int(block_off[-1]) + g,), payload, dtype=torch.int32, device=dev)
    wd = torch.full((g + r + g,), payload, dtype=torch.int32, device=dev)
    we = torch.full((2 * (g + t_rows + g),), payload, dtype=torch.int32, device=dev)
    eng.score_dense_pca_dev(xin.data_ptr() + 8 * g, offsets, 0.5, ws.data_ptr() + 4 * g, block_off, wd.data_ptr() + 4 * g,
                            we.data_ptr() + 8 * g)
    torch.cuda.synchronize()
    s, dd, ee = ws.cpu().numpy(), wd.cpu().numpy(), we.cpu().numpy().reshape(-1, 2)
    inside = np.zeros(s.size, bool)
    for q, n in enumerate(sizes):
        inside[g + block_off[q]:g + block_off[q] + n * n] = True
    assert (s[~inside] == payload).all(), "a store outside the blocks"
    assert not (s[inside] == payload).any(), "a block element left unwritten"
    assert (dd[:g] == payload).all() and (dd[g + r:] == payload).all() and not (dd[g:g + r] == payload).any()
    assert (ee[:g] == payload).all() and (ee[g + t_rows:] == payload).all() and not (ee[g:g + t_rows] == payload).all(1).any()
    blocks, info = diarize.score_dense_pca(eng, x, offsets, 0.5, return_info=True)
    for q, n in enumerate(sizes):
        got = s[g + block_off[q]:g + block_off[q] + n * n].view(np.float32).reshape(n, n)
        assert np.array_equal(got.view(np.uint32), blocks[q].view(np.uint32))
    assert np.array_equal(dd[g:g + r], info["dims"])
    # the clustering form: its five outputs between guards
    outs = {k: torch.full((g + n + g,), payload, dtype=torch.int32, device=dev)
            for k, n in (("l", t_rows), ("k", r), ("a", t_rows - r), ("b", t_rows - r), ("c", 2 * (t_rows - r)))}
    ptr = {k: v.data_ptr() + 4 * g for k, v in outs.items()}
    eng.score_dense_pca_ahc_dev(xin.data_ptr() + 8 * g, offsets, 0.5, 0, 0.0, np.ones(r, np.int32), ptr["l"], ptr["k"], ptr["a"],
                                ptr["b"], ptr["c"])
    torch.cuda.synchronize()
    want = diarize.ahc(eng, blocks, None, 1, True)
    for k, n in (("l", t_rows), ("k", r), ("a", t_rows - r), ("b", t_rows - r), ("c", 2 * (t_rows - r))):
        w = outs[k].cpu().numpy()
        assert (w[:g] == payload).all() and (w[g + n:] == payload).all(), k
    assert np.array_equal(outs["l"].cpu().numpy()[g:g + t_rows], want[0])
    assert np.array_equal(outs["k"].cpu().numpy()[g:g + r], want[1])
    assert np.array_equal(outs["a"].cpu().numpy()[g:g + t_rows - r], want[2][0])
    assert np.array_equal(outs["c"].cpu().numpy()[g:g + 2 * (t_rows - r)].view(np.float64), want[2][2])


def test_create_call_destroy_gives_back_every_byte():
    from plda_amd import diarize
    from plda_amd import _native as N
    lib = N.load()
    sizes = [20, 130, 3]
    model, x, offsets = dm.case(61, sizes, 112, 0.3)
    gc.collect()
    first = lib.plda_device_bytes_held()
    for cycle in range(10):
        eng = _engine(model)
        diarize.score_dense_pca(eng, x, offsets, 0.3)
        diarize.ahc_dense_pca(eng, x, offsets, 0.3, 0.0)
        assert lib.plda_device_bytes_held() > first
        del eng
        gc.collect()
        held = lib.plda_device_bytes_held()
        assert held == first, "cycle %d: %d bytes of device memory not given back" % (cycle, held - first)


# ------------------------------------------------------------------------------------------------------ seeded sweep
def _sweep_cases():
    rng = np.random.default_rng(20260119)
    cases = []
    for i in range(20):
        d = int(rng.choice([5, 16, 33, 64, 100, 101, 128, 200]))
        r = int(rng.integers(1, 7))
        hi = int(rng.choice([4, 40, 150, 260]))
        sizes = tuple(int(v) for v in rng.integers(1, hi + 1, r))
        target = float(np.round(rng.uniform(0.05, 0.9), 3))
        cases.append(pytest.param(1000 + i, sizes, d, target, id="%d-D%d-N%d-t%g" % (i, d, max(sizes), target)))
    return cases


@pytest.mark.parametrize("seed,sizes,d,target", _sweep_cases())
def test_seeded_sweep(seed, sizes, d, target):
    model, x, offsets = dm.case(seed, sizes, d, target)
    _parity(_engine(model), model, x, offsets, target)
