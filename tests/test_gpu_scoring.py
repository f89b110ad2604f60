"""GPU parity: trials matrix / trial list / transform / z-norm vs the fp64 oracle.

All calls go through the C ABI (plda_amd.MPlda -> ctypes -> libplda_hip.so).
Reference behaviour under test: src/pldamodule.cpp:111-277.
"""
import numpy as np
import pytest

from conftest import make_data, score_tol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from plda_amd import MPlda
    return MPlda(0)


def _model(oracle, seed, n, d, k, **kw):
    x, y = make_data(seed, n, d, k, **kw)
    return oracle.fit(x, y, 5), x, y


def _load(engine, m):
    engine.set_model(m["mean"], m["transform"], m["psi"])


@pytest.mark.parametrize("d,m_rows,nt", [(200, 300, 517), (64, 128, 128), (10, 7, 1000), (33, 129, 257), (150, 1, 1)])
@pytest.mark.parametrize("n_enrol", [1, 7])
def test_score_matrix_uniform(engine, oracle, d, m_rows, nt, n_enrol):
    m, x, y = _model(oracle, 11, 40 * 30, d, 40, scale_between=0.3)
    _load(engine, m)
    rng = np.random.default_rng(5)
    U = np.stack([oracle.transform_ivector(m, r, n_enrol) for r in rng.random((m_rows, d)) + 0.2])
    V = np.stack([oracle.transform_ivector(m, r, 1) for r in rng.random((nt, d))])
    ref = oracle.score_block(m["psi"], U, n_enrol, V)
    got = engine.score_matrix((n_enrol, U), (1, V))
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert (np.abs(got - ref) <= score_tol(ref)).all(), np.abs(got - ref).max()


def test_score_matrix_mixed_counts(engine, oracle):
    d = 96
    m, x, y = _model(oracle, 12, 2000, d, 50, skew=True, scale_between=0.5)
    _load(engine, m)
    rng = np.random.default_rng(6)
    counts = rng.integers(1, 6, 211).astype(np.int32)
    U = np.stack([oracle.transform_ivector(m, r, c) for r, c in zip(rng.random((211, d)), counts)])
    V = np.stack([oracle.transform_ivector(m, r, 1) for r in rng.random((333, d))])
    ref = oracle.score_block(m["psi"], U, counts, V)
    got = engine.score_matrix((counts, U), (1, V))
    assert (np.abs(got - ref) <= score_tol(ref)).all(), np.abs(got - ref).max()


def test_transposed_b_detected(engine, oracle):
    """asymmetric operands: a transposed tile or swapped row/col bias cannot pass."""
    d = 40
    m, _, _ = _model(oracle, 13, 600, d, 20, scale_between=1.0)
    _load(engine, m)
    U = np.zeros((130, d)); V = np.zeros((70, d))
    U[np.arange(130), np.arange(130) % d] = 1.0 + np.arange(130) / 7.0
    V[np.arange(70), (3 * np.arange(70)) % d] = -2.0 + np.arange(70) / 5.0
    ref = oracle.score_block(m["psi"], U, 3, V)
    got = engine.score_matrix((3, U), (1, V))
    assert (np.abs(got - ref) <= score_tol(ref)).all()


def test_score_pairs_and_scalar_score(engine, oracle):
    d = 50
    m, x, y = _model(oracle, 14, 900, d, 30, skew=True, scale_between=0.4)
    _load(engine, m)
    el, ec, ev = oracle.transform_groups(m, x[:200], y[:200])
    tl, tc, tv = oracle.transform_groups(m, x[200:300], np.arange(100, dtype=np.uint64))
    rng = np.random.default_rng(1)
    e = rng.integers(0, len(el), 500); t = rng.integers(0, 100, 500)
    ref = np.array([oracle.llr(m["psi"], ev[a], ec[a], tv[b]) for a, b in zip(e, t)])
    got = engine.score_trials((ec, ev), (tc, tv), e, t)
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-11)
    s = engine.score(int(el[3]), (int(ec[3]), ev[3]), (1, tv[5]))
    assert isinstance(s, float)
    assert abs(s - oracle.llr(m["psi"], ev[3], ec[3], tv[5])) < 1e-10


def test_transform_groups_matches_oracle(engine, oracle):
    d = 72
    m, x, y = _model(oracle, 15, 1500, d, 60, skew=True, scale_between=0.2)
    _load(engine, m)
    labels = (y[:700] * 7919 + 13).astype(np.uint64)      # non-dense, large label values
    got = engine.transform(x[:700], labels)
    rl, rc, rv = oracle.transform_groups(m, x[:700], labels)
    assert list(got.keys()) == [int(v) for v in rl]         # ascending label order (:164)
    for i, k in enumerate(rl):
        n, vec = got[int(k)]
        assert n == rc[i] and vec.dtype == np.float64
        np.testing.assert_allclose(vec, rv[i], rtol=1e-13, atol=1e-13 * np.abs(rv[i]).max())
    # the rule of tests/transform_model.py against the longdouble definition on the longdouble group means: every element within
    # its derived bound, the length-norm invariant sum t^2 / (psi + 1/n) = D to (D + 24) u (it was held to 1e-8)
    import transform_model as TM
    from test_gpu_transform_edges import _groups_reference
    keys, counts, ref = _groups_reference((m["mean"], m["transform"], m["psi"]), x[:700], labels)
    TM.assert_well_posed(ref)
    assert keys.tolist() == [int(v) for v in rl] and counts.tolist() == [int(c) for c in rc]
    TM.assert_rule(np.stack([got[int(k)][1] for k in keys]), ref, m["psi"], counts, "transform_groups")


def test_znorm_stats_and_normalised_scores(engine, oracle):
    d = 48
    m, x, y = _model(oracle, 16, 1200, d, 40, scale_between=0.5)
    from plda_amd import MPlda
    eng = MPlda(0)
    _load(eng, m)
    enrol = eng.transform(x[:160], y[:160])
    ids = list(enrol.keys())
    models = np.stack([enrol[k][1] for k in ids])
    bkg = x[300:300 + 391]
    rm, rs = oracle.norm(m, bkg, models)
    assert eng.norm(bkg, enrol) is None
    zm, zs = eng.znorm_stats()
    gm = np.array([zm[k] for k in ids]); gs = np.array([zs[k] for k in ids])
    assert (np.abs(gm - rm) <= 1e-10 * np.maximum(np.abs(rm), np.abs(rm).mean())).all(), np.abs(gm - rm).max()
    assert (np.abs(gs - rs) <= 1e-10 * rs).all(), (np.abs(gs - rs) / rs).max()
    # insert-once (quirk Q8): a second norm() on other data leaves the statistics alone
    eng.norm(x[700:900], enrol)
    zm2, _ = eng.znorm_stats()
    assert zm2 == zm
    # z-normalised trials matrix vs oracle with the ORACLE's statistics plugged in
    eng2 = MPlda(0); _load(eng2, m)
    eng2._meanz = {k: float(v) for k, v in zip(ids, rm)}
    eng2._stdvz = {k: float(v) for k, v in zip(ids, rs)}
    test = eng2.transform(x[500:620], np.arange(120, dtype=np.uint64))
    tv = np.stack([test[k][1] for k in test])
    counts = np.array([enrol[k][0] for k in ids], np.int32)
    ref = oracle.score_block(m["psi"], models, counts, tv, rm, rs)
    got = eng2.score_matrix(enrol, test)
    assert (np.abs(got - ref) <= score_tol(ref)).all(), np.abs(got - ref).max()
    s = eng2.score(ids[2], enrol[ids[2]], test[7])
    assert abs(s - ref[2, 7]) < 1e-9 * max(1.0, abs(ref[2, 7]))


def test_smooth_and_truncate(engine, oracle):
    d = 30
    m, x, y = _model(oracle, 17, 600, d, 20, scale_between=0.6)
    _load(engine, m)
    engine.smooth(0.5)
    sm = oracle.smooth(m, 0.5)
    g = engine.get_model()
    np.testing.assert_allclose(g["psi"], sm["psi"], rtol=1e-12)
    np.testing.assert_allclose(g["transform"], sm["transform"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(g["offset"], sm["offset"], rtol=1e-10, atol=1e-12)
    engine.smooth(0.0)  # identity
    np.testing.assert_allclose(engine.get_model()["psi"], sm["psi"], rtol=1e-15)
    engine.truncate(12)
    assert engine.dims() == (12, d)
    out = engine.transform_array(x[:5], 1)
    assert out.shape == (5, 12)


def test_trial_list_scoring_matches_per_call_score(engine, oracle):
    """scorePLDA.py's loop (one plda.score per trial) == one batched trial-list launch."""
    import io
    from liblda import PLDA
    from plda_amd import trials
    x, y = make_data(31, 600, 24, 12, scale_between=0.5)
    p = PLDA()
    p.fit(x, y, 4)
    enrol = p.transform(x[:120], y[:120])
    test = p.transform(x[120:150], np.arange(30, dtype=np.uint64))
    p.norm(x[200:280], enrol)
    names_e = {"m%d" % k: k for k in enrol}
    names_t = {"u-%d" % k: k for k in test}
    ref = {"m%d" % k: [["u-%d" % j, "m%d" % k] for j in (0, 7, 29)] for k in list(enrol)[:5]}
    out = io.StringIO()
    n, err = trials.score_trial_list(p, ref, enrol, test, names_e, names_t, out)
    assert (n, err) == (15, 0)
    lines = out.getvalue().splitlines()
    for line, (k, j) in zip(lines, [(k, j) for k in list(enrol)[:5] for j in (0, 7, 29)]):
        expect = "m%d m%d-u-%d %.3f" % (k, k, j, p.score(k, enrol[k], test[j]))
        assert line == expect


def test_sharded_scorer_on_device_tensors(engine, oracle):
    """plda_amd.sharding's tensor wrapper of plda_score_matrix_sharded_local_dev (world size 1 here; several ranks:
    tests/test_gpu_comm.py by emulation, tests/test_gpu_comm_procs.py between processes): the compact slab is the
    whole matrix, the row map the identity, and gather=True assembles the same matrix once more."""
    import torch
    from plda_amd.sharding import score_matrix_sharded
    d = 40
    m, x, y = _model(oracle, 19, 800, d, 25, scale_between=0.4)
    _load(engine, m)
    rng = np.random.default_rng(3)
    counts = rng.integers(1, 4, 150).astype(np.int32)
    U = np.stack([oracle.transform_ivector(m, r, c) for r, c in zip(rng.random((150, d)), counts)])
    V = np.stack([oracle.transform_ivector(m, r, 1) for r in rng.random((90, d))])
    dev = torch.device("cuda", 0)
    loc, rows, full = score_matrix_sharded(engine, torch.from_numpy(U).to(dev), torch.from_numpy(counts).to(dev),
                                           torch.from_numpy(V).to(dev), gather=True, block_rows=64)
    torch.cuda.synchronize()
    ref = oracle.score_block(m["psi"], U, counts, V)
    assert loc.shape == (150, 90) and rows.tolist() == list(range(150)) and torch.equal(full, loc)
    assert (np.abs(loc.cpu().numpy() - ref) <= score_tol(ref)).all()
    engine.set_stream(None)


@pytest.mark.parametrize("d,nb,nmodels", [(48, 391, 40), (200, 1000, 64), (206, 650, 4), (207, 600, 5), (208, 700, 3), (230, 520, 7), (10, 2, 4),
                                          (33, 1, 6), (64, 70, 9), (256, 2300, 6)])
@pytest.mark.parametrize("variant", ["0", "1", "2", "3"])
def test_znorm_statistics_both_arms(oracle, monkeypatch, d, nb, nmodels, variant):
    """MPlda_norm (pldamodule.cpp:196-256).  Arm 0 (default): statistics from the cohort's fp64 moments -- the LLR is
    bilinear in (cohort row, model) plus a bias on each side -- taken in ONE read of the transformed cohort (round 5:
    pilot shift + the (D + 2)-wide SYRK that forms its rows on the way into LDS), arm 2: the same moments in the five
    passes of rounds 2-4 (also what D + 2 > 208 takes); both held to 1e-10 against the oracle's explicit per-pair
    loop; arm 1: every LLR on the fp32 GEMM with the fused sum / sum-of-squares epilogue, held to the 1e-4 of
    north_star.  Shapes straddle the one-read kernel's limit (D + 2 = 208 | 209: beyond it arm 0 writes the shifted rows
    once and the block SYRK reads them once; 256 x 2300 reaches that SYRK), the older (D + 1)-wide SYRK's kernel choice, a cohort of 70 rows (the pilot takes 64) and the degenerate cohorts of one and two rows (std = 0 exactly
    for one row, as the reference's population std).  Arm 3: arm 0 with the model pass as a general GEMM + row kernel (rounds
    2-5) instead of the transform kernel's shape with the quadratic form in its epilogue (round 6; D <= 208)."""
    monkeypatch.setenv("PLDA_ZNORM_VARIANT", variant)
    from plda_amd import MPlda
    m, x, y = _model(oracle, 16, 1500, d, 30, scale_between=0.5)
    eng = MPlda(0)
    _load(eng, m)
    rng = np.random.default_rng(d + nb)
    bkg = rng.random((nb, d))
    models = np.stack([oracle.transform_ivector(m, r, 1) for r in rng.random((nmodels, d)) + 0.1])
    rm, rs = oracle.norm(m, bkg, models)
    enrol = {int(k): (1, models[k]) for k in range(nmodels)}
    eng.norm(bkg, enrol)
    zm, zs = eng.znorm_stats()
    gm = np.array([zm[k] for k in range(nmodels)]); gs = np.array([zs[k] for k in range(nmodels)])
    tol = 1e-10 if variant != "1" else 1e-4
    scale = np.maximum(np.abs(rm), np.abs(rm).mean())
    assert (np.abs(gm - rm) <= tol * scale).all(), (np.abs(gm - rm) / scale).max()
    if nb == 1:
        assert (gs == 0.0).all() if variant != "1" else (np.abs(gs) <= 1e-3 * scale).all()
    else:
        assert (np.abs(gs - rs) <= tol * np.maximum(rs, 1e-3 * scale)).all(), (np.abs(gs - rs) / rs).max()


@pytest.mark.parametrize("d", [1, 24, 200])
def test_llr_with_mixed_counts_against_the_closed_form_gaussian_ratio(monkeypatch, d):
    """The same known answer (scipy.stats, neither the oracle nor the engine's kernels) for enrol models with DIFFERENT
    utterance counts -- the bucketed form of the trials GEMM (one column-bias vector per distinct count) and the fp64
    trial-list kernel: per dimension the joint covariance of (enrol mean of n_i vectors, test vector) is
    [[psi + 1/n_i, psi], [psi, psi + 1]]."""
    from scipy.stats import norm
    from plda_amd import MPlda
    monkeypatch.delenv("PLDA_MIXED_VARIANT", raising=False)       # (the depth asserted below is the bucketed form's)
    rng = np.random.default_rng(300 + d)
    psi = np.sort(rng.random(d) * 5.0 + 1e-3)[::-1].copy()
    eng = MPlda(0)
    eng.set_model(np.zeros(d), np.eye(d), psi)
    m, nt = 37, 41
    n = rng.choice([1, 2, 5, 11], m).astype(np.int32)
    n[:4] = [1, 2, 5, 11]
    U, V = rng.standard_normal((m, d)) * 1.5, rng.standard_normal((nt, d)) * 1.5
    inv = 1.0 / n[:, None].astype(np.float64)
    cmean = (psi[None, :] / (psi[None, :] + inv))[:, None, :] * U[:, None, :]
    cvar = (psi[None, :] + 1.0 - psi[None, :] ** 2 / (psi[None, :] + inv))[:, None, :]
    ref = (norm.logpdf(V[None, :, :], cmean, np.sqrt(cvar)) - norm.logpdf(V[None, :, :], 0.0, np.sqrt(psi + 1.0))).sum(-1)
    got = eng.score_matrix((n, U), (1, V))
    assert eng.score_last_shape()[2] == d + 3                      # four distinct counts: three extra contraction columns
    assert (np.abs(got - ref) <= score_tol(ref)).all(), np.abs(got - ref).max()
    e, t = np.repeat(np.arange(m), nt), np.tile(np.arange(nt), m)
    lst = eng.score_trials((n, U), (1, V), e, t).reshape(m, nt)
    assert np.abs(lst - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("d,n_enrol", [(1, 1), (1, 4), (7, 3), (200, 1)])
def test_llr_against_the_closed_form_gaussian_ratio(d, n_enrol):
    """A known answer that is not the oracle: in the PLDA space (diagonal psi, unit within-class variance) the mean u
    of n enrolment vectors and a test vector v of the same speaker are jointly Gaussian with covariance
    [[psi + 1/n, psi], [psi, psi + 1]] per dimension, so  LLR = sum_d log N(v_d | psi u_d / (psi + 1/n),
    psi + 1 - psi^2 / (psi + 1/n)) - log N(v_d | 0, psi + 1)  (Plda::LogLikelihoodRatio, pldamodule.cpp:266).
    Both the fp32 GEMM matrix and the fp64 trial-list kernel must give it."""
    from scipy.stats import norm
    from plda_amd import MPlda
    rng = np.random.default_rng(100 + d)
    psi = np.sort(rng.random(d) * 5.0 + 1e-3)[::-1].copy()
    eng = MPlda(0)
    eng.set_model(np.zeros(d), np.eye(d), psi)
    U, V = rng.standard_normal((33, d)) * 1.5, rng.standard_normal((41, d)) * 1.5
    cmean = (psi / (psi + 1.0 / n_enrol))[None, None, :] * U[:, None, :]
    cvar = psi + 1.0 - psi * psi / (psi + 1.0 / n_enrol)
    ref = (norm.logpdf(V[None, :, :], cmean, np.sqrt(cvar)) - norm.logpdf(V[None, :, :], 0.0, np.sqrt(psi + 1.0))).sum(-1)
    got = eng.score_matrix((n_enrol, U), (1, V))
    assert (np.abs(got - ref) <= score_tol(ref)).all(), np.abs(got - ref).max()
    e, t = np.repeat(np.arange(33), 41), np.tile(np.arange(41), 33)
    lst = eng.score_trials((np.full(33, n_enrol, np.int32), U), (1, V), e, t).reshape(33, 41)
    assert np.abs(lst - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max())


def test_znorm_statistics_against_the_closed_form():
    """norm() against numbers that come from neither the oracle nor the engine's own kernels: with T = I, mean = 0 the
    cohort rows are only length-normalised (Plda::TransformIvector with num_examples = Nb, pldamodule.cpp:224:
    x * sqrt(D / sum x^2 / (psi + 1/Nb))), every (cohort row as 1-utterance enrolment, model as test) LLR is the
    closed-form Gaussian ratio of the test above, and the statistics are their mean and POPULATION std per model."""
    from scipy.stats import norm
    from plda_amd import MPlda
    rng = np.random.default_rng(77)
    d, nb, nm = 24, 300, 17
    psi = np.sort(rng.random(d) * 3.0 + 0.05)[::-1].copy()
    eng = MPlda(0)
    eng.set_model(np.zeros(d), np.eye(d), psi)
    bkg = rng.standard_normal((nb, d))
    models = rng.standard_normal((nm, d)) * 1.3
    t = bkg * np.sqrt(d / (bkg * bkg / (psi + 1.0 / nb)).sum(1))[:, None]
    cmean = (psi / (psi + 1.0))[None, None, :] * t[:, None, :]
    cvar = psi + 1.0 - psi * psi / (psi + 1.0)
    llr = (norm.logpdf(models[None, :, :], cmean, np.sqrt(cvar)) - norm.logpdf(models[None, :, :], 0.0, np.sqrt(psi + 1.0))).sum(-1)
    rm, rs = llr.mean(0), llr.std(0)
    eng.norm(bkg, {int(k): (1, models[k]) for k in range(nm)})
    zm, zs = eng.znorm_stats()
    gm = np.array([zm[k] for k in range(nm)]); gs = np.array([zs[k] for k in range(nm)])
    assert np.abs(gm - rm).max() <= 1e-10 * np.abs(rm).max(), np.abs(gm - rm).max()
    assert (np.abs(gs - rs) <= 1e-9 * rs).all(), (np.abs(gs - rs) / rs).max()


@pytest.mark.parametrize("variant", ["0", "1"])
@pytest.mark.parametrize("din,dout", [(7, 7), (77, 77), (128, 128), (129, 129), (200, 200), (200, 150), (209, 209),
                                      (256, 256), (257, 257), (300, 300), (385, 385), (512, 512), (512, 200),
                                      (520, 520)])
def test_transform_rows_all_dimension_classes(din, dout, variant, monkeypatch):
    """K4 through every instantiation of the one-pass kernel -- the five dimension classes, each with its main block shape
    (row counts above one round of the persistent grid: 33 017) and its 64 / 32 / 16-row tail shapes (12 000 / 5 000 /
    <= 1 000 rows) -- and the GEMM + length-norm pair behind it (Dout > 512, or PLDA_TRANSFORM_VARIANT=1): ragged row
    counts, K not a multiple of 16 or of 4, truncated models (Dout < Din), per-row and uniform counts, against the longdouble
    model of TransformIvector's definition (pldamodule.cpp:171 -> Plda::TransformIvector; tests/transform_model.py).  Which
    shapes a CU count really reaches is asserted by name in tests/test_gpu_transform_edges.py."""
    import transform_model as TM
    from plda_amd import MPlda
    monkeypatch.setenv("PLDA_TRANSFORM_VARIANT", variant)
    rng = np.random.default_rng(din * 1000 + dout)
    q, _ = np.linalg.qr(rng.standard_normal((din, din)))
    T = (q * (0.5 + rng.random(din))[:, None])[:dout]
    mean = rng.random(din)
    psi = np.sort(rng.random(dout) * 3.0 + 0.01)[::-1].copy()
    eng = MPlda(0)
    eng.set_model(mean, T, psi)
    for r in (1, 63, 64, 129, 1000) + ((5000, 12000, 33017) if variant != "1" or din == 200 else ()):
        x = rng.standard_normal((r, din))
        n = rng.integers(1, 9, r).astype(np.int32)
        for ne in (3, n):
            got = eng.transform_array(x, ne)
            # the rule of tests/transform_model.py, against the longdouble DEFINITION T (x - mean) -- and never looser than the
            # flat band rtol = 1e-11, atol = 1e-12 this test held against the NumPy restatement of the device's own formula
            plan = eng.transform_plan(r)
            TM.assert_rule_many(got, T, mean, psi, x, ne, "%dx%d R = %d" % (din, dout, r), also=(plan["main_rows"] - 1, plan["main_rows"]),
                                no_looser_than=(1e-11, 1e-12))


def test_prepared_test_side_is_reused_and_invalidated():
    """plda_score_prepare_dev: the test side packed once gives matrices bit-identical to an unprepared call's for every
    later enrol slab (uniform counts; mixed counts in the form that was prepared), and the reuse ends when the test rows,
    the count kind or the model change."""
    import torch
    from plda_amd import MPlda
    dev = torch.device("cuda", 0)
    d, m, nt = 56, 700, 1300
    rng = np.random.default_rng(21)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    eng = MPlda(0)
    eng.set_model(rng.random(d), q * (1.0 + rng.random(d))[:, None], np.sort(rng.random(d) * 4.0 + 0.05)[::-1].copy())
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    U = torch.from_numpy(rng.standard_normal((m, d))).to(dev)
    V = torch.from_numpy(rng.standard_normal((nt, d))).to(dev)
    V2 = torch.from_numpy(rng.standard_normal((nt, d))).to(dev)
    n = torch.from_numpy(rng.integers(1, 6, m).astype(np.int32)).to(dev)

    def score(dn, nu, Vt):
        o = torch.empty((m, nt), dtype=torch.float32, device=dev)
        eng.score_matrix_dev(U.data_ptr(), dn.data_ptr() if dn is not None else None, nu, m, Vt.data_ptr(), nt, o.data_ptr(), nt)
        torch.cuda.synchronize()
        return o

    ref_u, ref_m = score(None, 2, V), score(n, 0, V)
    ref_u2 = score(None, 2, V2)
    eng.score_prepare_dev(V.data_ptr(), nt, mixed_counts=False, n_uniform=2)
    assert torch.equal(score(None, 2, V), ref_u) and torch.equal(score(None, 2, V), ref_u)      # reused, twice
    eng.score_prepare_counts_dev(V.data_ptr(), nt, [1, 2, 3, 4, 5])                              # the bucketed form (what an unprepared call uses)
    assert torch.equal(score(n, 0, V), ref_m) and torch.equal(score(n, 0, V), ref_m)
    eng.score_prepare_dev(V.data_ptr(), nt, mixed_counts=True)                                   # the depth-2D form: other bits, same scores
    m2d = score(n, 0, V)
    assert torch.equal(score(n, 0, V), m2d) and float((m2d - ref_m).abs().max()) < 1e-3
    # the reuse is real, and guarded: the cache is keyed on the pointer, so overwriting the rows behind it -- an in-place
    # update, or an allocator handing the address to another tensor -- must not score against the stale packing.  Round 4
    # FAILED such a call (content fingerprint of 64 sampled rows); since round 5 the mismatch is a cache MISS: the rows are
    # packed again and the call returns the new rows' scores (advisor, round 4: a legitimate tensor at a recycled address).
    eng.score_prepare_dev(V.data_ptr(), nt, mixed_counts=False, n_uniform=2)
    keep = V.clone()
    V.copy_(V2)
    torch.cuda.synchronize()
    assert torch.equal(score(None, 2, V), ref_u2)
    assert torch.equal(score(None, 2, V), ref_u2)
    # a change in ONE sampled row (the last) is enough
    eng.score_prepare_dev(V.data_ptr(), nt, mixed_counts=False, n_uniform=2)
    V[-1, 0] += 1.0
    torch.cuda.synchronize()
    changed = score(None, 2, V)
    assert torch.equal(changed[:, :-1], ref_u2[:, :-1]) and not torch.equal(changed[:, -1], ref_u2[:, -1])
    V.copy_(V2)
    # anything in the key changes -> repacked silently: another count, the other kind of counts, unprepare, the model
    eng.score_prepare_dev(V.data_ptr(), nt, mixed_counts=False, n_uniform=2)
    assert torch.equal(score(None, 3, V), score(None, 3, V2))
    eng.score_prepare_dev(V.data_ptr(), nt, mixed_counts=False, n_uniform=2)
    assert torch.equal(score(None, 2, V), ref_u2)
    V.copy_(keep)
    eng.score_unprepare()
    assert torch.equal(score(None, 2, V), ref_u)
    eng.score_prepare_dev(V.data_ptr(), nt, mixed_counts=False, n_uniform=2)
    eng.smooth(0.5)                                         # model epoch moves on: no reuse, hence no fingerprint check either
    V.copy_(V2)
    torch.cuda.synchronize()
    one = MPlda(0)
    mdl = eng.get_model()
    one.set_model(mdl["mean"], mdl["transform"], mdl["psi"])
    one.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    o1 = torch.empty((m, nt), dtype=torch.float32, device=dev)
    one.score_matrix_dev(U.data_ptr(), None, 2, m, V2.data_ptr(), nt, o1.data_ptr(), nt)
    torch.cuda.synchronize()
    assert torch.equal(score(None, 2, V), o1)
    eng.set_stream(None)


@pytest.mark.parametrize("d,m,nt,n_enrol", [(200, 300, 517, 1), (200, 2049, 1100, 7), (7, 65, 64, 3), (1, 5, 700, 1), (129, 64, 1, 2),
                                            (512, 130, 257, 100), (263, 1000, 129, 4), (64, 200, 33000, 2), (40, 33000, 100, 1)])
@pytest.mark.parametrize("znorm", [False, True])
def test_one_pass_prep_bit_identical(monkeypatch, d, m, nt, n_enrol, znorm):
    """prep_side_kernel (one pass over a side's rows: bias, bias pair and packed operand) against the separate
    weighted_sq_bias / pack / bias_pairs kernels (PLDA_PREP_VARIANT=1): same per-lane order of the weighted sum, same
    butterfly, same operand arithmetic -- the trials matrix is BIT-identical, with and without the z-norm map folded into
    the enrol side (a zero zstd leaves its row unscaled in both)."""
    import torch
    from plda_amd import MPlda
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7 * d + m)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    model = (rng.random(d), q * (1.0 + rng.random(d))[:, None], np.sort(rng.random(d) * 4.0 + 0.05)[::-1].copy())
    U = torch.from_numpy(rng.standard_normal((m, d))).to(dev)
    V = torch.from_numpy(rng.standard_normal((nt, d))).to(dev)
    zm = torch.from_numpy(rng.standard_normal(m)).to(dev)
    zs = torch.from_numpy(rng.random(m) + 0.5).to(dev)
    zs[m // 2] = 0.0
    outs = []
    # 2 / 3: prep_side_kernel with 16 / 4 rows per wave; the product (0) picks by row count -- two short sides (<= 32 768 rows) share
    # ONE launch (prep_both_kernel), a short and a long side take one kernel each
    for variant in ("0", "1", "2", "3"):
        monkeypatch.setenv("PLDA_PREP_VARIANT", variant)
        eng = MPlda(0)
        eng.set_model(*model)
        o = torch.full((m, nt + 3), -7.0, dtype=torch.float32, device=dev)
        eng.score_matrix_dev(U.data_ptr(), None, n_enrol, m, V.data_ptr(), nt, o.data_ptr(), nt + 3,
                             zm.data_ptr() if znorm else None, zs.data_ptr() if znorm else None)
        torch.cuda.synchronize()
        outs.append(o)
    for o in outs[1:]:
        assert torch.equal(outs[0], o)
    assert bool((outs[0][:, nt:] == -7.0).all()) and bool(torch.isfinite(outs[0][:, :nt]).all())


def test_uniform_coefficients_follow_count_and_model(oracle):
    """The per-dimension coefficients of the uniform-count path are kept on the device across calls, keyed by (model, count,
    dimension), and so are the bucket tables of a mixed-count call, keyed by the set of counts; both live in one buffer: another
    count, another set, the other kind of call in between, set_model and smooth each must be seen -- every call equals the oracle, and a fresh engine's bits."""
    from plda_amd import MPlda
    d, m, nt = 72, 300, 517
    rng = np.random.default_rng(5)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    counts = rng.integers(1, 4, m).astype(np.int32)
    eng = MPlda(0)
    models = [(rng.random(d), q * (1.0 + rng.random(d))[:, None], np.sort(rng.random(d) * 4.0 + 0.05)[::-1].copy()) for _ in range(2)]
    for mean, T, psi in models:
        eng.set_model(mean, T, psi)
        counts2 = np.where(counts == 2, 7, counts).astype(np.int32)      # another set of distinct counts: {1, 3, 7}
        for n in (2, 2, 5, counts, counts, 5, counts2, counts, 2):
            got = eng.score_matrix((n, U), (1, V))
            ref = oracle.score_block(psi, U, n, V)
            assert (np.abs(got - ref) <= score_tol(ref)).all(), (n if np.isscalar(n) else "mixed", np.abs(got - ref).max())
            fresh = MPlda(0)
            fresh.set_model(mean, T, psi)
            assert np.array_equal(fresh.score_matrix((n, U), (1, V)), got)
    eng.smooth(0.3)
    fresh = MPlda(0)
    fresh.set_model(*models[1])
    fresh.smooth(0.3)
    assert np.array_equal(fresh.score_matrix((2, U), (1, V)), eng.score_matrix((2, U), (1, V)))


@pytest.mark.parametrize("dout", [200, 197, 193])
def test_transform_c2_shape_rounds_and_tails(dout):
    """K4 at the C2 shape (Din = 200, a uniform count) against the longdouble model of TransformIvector: exactly one round
    of the persistent grid, whole rounds plus a 32-row and a 16-row tail launch; truncated models put the edge of the
    output inside the thirteenth column tile; one row of another magnitude (the norm is per row)."""
    import transform_model as TM
    from plda_amd import MPlda
    din = 200
    rng = np.random.default_rng(900 + dout)
    q, _ = np.linalg.qr(rng.standard_normal((din, din)))
    T = (q * (0.5 + rng.random(din))[:, None])[:dout]
    mean = rng.random(din)
    psi = np.sort(rng.random(dout) * 3.0 + 0.01)[::-1].copy()
    eng = MPlda(0)
    eng.set_model(mean, T, psi)
    for r, ne in ((32768, 1), (40011, 7), (100000, 3)):
        x = rng.standard_normal((r, din))
        x[r // 3] *= 1e3                                   # one row of another magnitude: the norm is per row
        got = eng.transform_array(x, ne)
        # the rule of tests/transform_model.py against the longdouble definition, never looser than the flat band rtol = 1e-12,
        # atol = 1e-13 this test held against the NumPy restatement; the plan says which launches these rows took
        plan = eng.transform_plan(r)
        assert (plan["arm"], plan["cls"], plan["main_block"]) == ("fused", 1, 128)
        if plan["cus"] == 256:
            assert (plan["main_rows"], plan["tail_block"]) == {32768: (32768, 0), 40011: (32768, 32), 100000: (98304, 16)}[r]
        TM.assert_rule_many(got, T, mean, psi, x, ne, "C2 %d R = %d" % (dout, r), also=(r // 3, plan["main_rows"] - 1, plan["main_rows"]),
                            no_looser_than=(1e-12, 1e-13))


@pytest.mark.parametrize("d,kind", [(50, "mixed"), (200, "uniform"), (129, "many"), (64, "beyond")])
def test_long_trial_lists_run_on_per_count_tables(monkeypatch, oracle, d, kind):
    """plda_score_pairs on a list of >= 16 384 trials: the terms of Plda::LogLikelihoodRatio (pldamodule.cpp:266) that depend on
    (enrol count, dimension) only come from per-count tables instead of four divisions and two logarithms per element.  Same
    numbers: against the oracle's per-trial LLR on a sample (1e-10 relative, as the short lists are held to), against the
    verbatim kernel (PLDA_MIXED_VARIANT=1 keeps it) on the whole list, with and without z-norm statistics; counts the tables do
    not take (> 4095) stay verbatim."""
    from plda_amd import MPlda
    rng = np.random.default_rng(d)
    m, nt, p = 700, 3000, 40000
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    model = (rng.random(d), q * (1.0 + rng.random(d))[:, None], np.sort(rng.random(d) * 4.0 + 0.05)[::-1].copy())
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    vals = {"mixed": np.arange(1, 6), "uniform": np.array([3]), "many": rng.choice(np.arange(1, 300), 40, replace=False),
            "beyond": np.array([1, 5000])}[kind]
    counts = vals[rng.integers(0, len(vals), m)].astype(np.int32)
    e, t = np.sort(rng.integers(0, m, p)), rng.integers(0, nt, p)
    ids = np.arange(m, dtype=np.int64)
    outs = {}
    for arm in ("", "1"):
        if arm:
            monkeypatch.setenv("PLDA_MIXED_VARIANT", arm)
        else:
            monkeypatch.delenv("PLDA_MIXED_VARIANT", raising=False)
        eng = MPlda(0)
        eng.set_model(*model)
        plain = eng.score_trials((counts, U, ids), (1, V), e, t)
        eng._meanz = {int(k): -30.0 + 0.01 * k for k in ids}
        eng._stdvz = {int(k): 2.0 + 0.001 * k for k in ids}
        eng._stdvz[5] = 0.0                       # (a zero std leaves the row's trials un-normalised)
        outs[arm] = (plain, eng.score_trials((counts, U, ids), (1, V), e, t))
    for a, b in zip(outs[""], outs["1"]):
        np.testing.assert_allclose(a, b, rtol=1e-11, atol=1e-11)
    sel = rng.integers(0, p, 300)
    ref = np.array([oracle.llr(model[2], U[e[i]], counts[e[i]], V[t[i]]) for i in sel])
    np.testing.assert_allclose(outs[""][0][sel], ref, rtol=1e-10, atol=1e-11)
    zref = np.array([r if e[i] == 5 else (r - (-30.0 + 0.01 * e[i])) / (2.0 + 0.001 * e[i]) for r, i in zip(ref, sel)])
    np.testing.assert_allclose(outs[""][1][sel], zref, rtol=1e-10, atol=1e-11)
    # an index outside the sets is an error code (found on the device for long lists), never a fault; the handle stays usable
    bad_t = t.copy(); bad_t[31000] = nt
    from plda_amd._native import PldaError
    with pytest.raises(PldaError, match="31000"):
        eng.score_trials((counts, U, ids), (1, V), e, bad_t)
    bad_e = e.copy(); bad_e[7] = -1
    with pytest.raises(PldaError, match="trial 7 "):
        eng.score_trials((counts, U, ids), (1, V), bad_e, t)
    np.testing.assert_array_equal(eng.score_trials((counts, U, ids), (1, V), e, t), outs["1"][1])


@pytest.mark.parametrize("nt", [1, 257])
def test_znorm_error_bound_when_the_cohort_spread_is_small(oracle, nt):
    """z = (raw - zmean) / zstd (src/pldamodule.cpp:269-273) multiplies the fp32 contraction's ABSOLUTE error by 1 / zstd: a
    cohort of near-identical rows gives a small zstd, and where raw ~ zmean the reference's z is ~ 0, so a bound relative to |z|
    alone cannot hold (round-5 stress sweep: 1e-6 .. 2.6e-4 absolute at Nt = 1 where the reference is exactly 0).  The bound
    that does hold, pinned here and stated in INTEGRATION.md "Divergences":
        |z_gpu - z_ref| <= 1e-4 max(|z|, mean|z|) + 4e-6 (1 + |raw|) / zstd."""
    from plda_amd import MPlda
    d = 64
    m, x, y = _model(oracle, 23, 1500, d, 50, scale_between=0.5)
    eng = MPlda(0)
    _load(eng, m)
    # one utterance per model: norm() scores the cohort with the roles swapped and n = 1 (pldamodule.cpp:235), so with n = 1 on
    # the enrol side too a test vector inside the cohort has raw ~ zmean, i.e. z ~ 0
    enrol = eng.transform(x[:60], np.arange(60, dtype=np.uint64))
    ids = list(enrol.keys())
    models = np.stack([enrol[k][1] for k in ids])
    counts = np.array([enrol[k][0] for k in ids], np.int32)
    rng = np.random.default_rng(9)
    base = x[700]
    bkg = base + 2e-3 * rng.standard_normal((300, d))             # a cohort of near-identical rows: tiny per-model spread
    rm, rs = oracle.norm(m, bkg, models)
    assert rs.max() < 0.2 and rs.min() > 0
    eng._meanz = {k: float(v) for k, v in zip(ids, rm)}
    eng._stdvz = {k: float(v) for k, v in zip(ids, rs)}
    # test vectors: cohort members exactly as norm() transformed them (num_examples = cohort rows, pldamodule.cpp:224; the
    # one-utterance LLR is symmetric, so raw ~ zmean and the reference's z is ~ 0), plus ordinary test vectors
    inside = np.stack([oracle.transform_ivector(m, bkg[i], bkg.shape[0]) for i in range(max(nt // 2, 1))])
    ordinary = np.stack([oracle.transform_ivector(m, r, 1) for r in x[800:800 + nt]])
    tv = np.concatenate([inside, ordinary])[:nt]
    test = (1, tv)
    raw = oracle.score_block(m["psi"], models, counts, tv)
    ref = oracle.score_block(m["psi"], models, counts, tv, rm, rs)
    got = eng.score_matrix(enrol, test)
    bound = 1e-4 * np.maximum(np.abs(ref), np.abs(ref).mean()) + 4e-6 * (1.0 + np.abs(raw)) / rs[:, None]
    err = np.abs(got - ref)
    assert (err <= bound).all(), (float(err.max()), float((err / bound).max()))
    # the cohort members' z really are O(1) (inside the cohort) while |raw| is tens: the regime the additive term is for
    k_in = min(inside.shape[0], nt)
    assert np.abs(ref[:, :k_in]).max() < 10.0 and np.abs(raw).max() > 10.0
    print("znorm bound: max err %.3g, max err/bound %.3g, zstd min %.3g, |raw| max %.3g" % (err.max(), (err / bound).max(), rs.min(), np.abs(raw).max()))


@pytest.mark.parametrize("d,nmodels", [(64, 40000), (128, 33100), (200, 36000)])
def test_znorm_model_pass_main_block_shapes(oracle, d, nmodels):
    """norm()'s model pass (round 6: x^T C x + lin . x and the mean from the transform kernel's epilogue) with enough models for
    its persistent main launch (128-row blocks on every CU: 8 column tiles per wave up to D = 128, 13 up to 208) AND a tail
    launch; every model against the oracle's explicit per-pair loop over a small cohort."""
    from plda_amd import MPlda
    m, x, y = _model(oracle, 31, 1200, d, 30, scale_between=0.5)
    eng = MPlda(0)
    _load(eng, m)
    rng = np.random.default_rng(d)
    bkg = rng.random((90, d))
    base = np.stack([oracle.transform_ivector(m, r, 1) for r in rng.random((500, d)) + 0.1])
    models = base[rng.integers(0, 500, nmodels)] * (1.0 + 0.05 * rng.standard_normal((nmodels, 1)))
    rm, rs = oracle.norm(m, bkg, models)
    eng.norm(bkg, {int(k): (1, models[k]) for k in range(nmodels)})
    dm, ds = eng.znorm_stats()
    zm = np.array([dm[k] for k in range(nmodels)]); zs = np.array([ds[k] for k in range(nmodels)])
    scale = np.maximum(np.abs(rm), np.abs(rm).mean())
    assert (np.abs(zm - rm) <= 1e-10 * scale).all(), (np.abs(zm - rm) / scale).max()
    assert (np.abs(zs - rs) <= 1e-10 * np.maximum(rs, 1e-3 * scale)).all(), (np.abs(zs - rs) / rs).max()
