"""GPU: guard bands around caller memory for the device-pointer entry points of MPlda.

Every input is a view inside a larger torch buffer whose neighbours -- at least 64 KiB before and after, and the tail of each
row where the call takes a leading dimension -- hold NaN; every output is a view inside a buffer pre-filled with the NaN
payload 0x7FC0DEAD (as int32 words), with guards before, after and between rows.  After the call the guards must still hold
their fill, compared as integers word for word (no store outside the output), no output word may still hold it (no element
left unwritten), and the outputs must be bit-identical to a run whose neighbours are zero (no read past an input reaches the
result).  Stray stores land in memory the test owns: these tests detect, they do not provoke."""
import numpy as np
import pytest

from conftest import make_data

pytestmark = pytest.mark.gpu

GUARD_BYTES = 64 << 10
PAYLOAD = 0x7FC0DEAD


def _dev():
    import torch
    return torch.device("cuda", 0)


def _input(a, nan, ld=None):
    """`a` (2-D, or 1-D) placed in a buffer with GUARD_BYTES of NaN (or zero) on both sides; rows `ld` apart when given."""
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a)
    g = GUARD_BYTES // a.itemsize
    rows, cols = (a.shape[0], a.shape[1]) if a.ndim == 2 else (1, a.shape[0])
    ld = ld or cols
    buf = torch.empty(g + rows * ld + g, dtype=t.dtype, device=_dev())
    if t.dtype.is_floating_point:
        buf.fill_(float("nan") if nan else 0.0)
    else:
        buf.fill_(-1 if nan else 0)              # (an index that points nowhere)
    body = buf[g:g + rows * ld].view(rows, ld)[:, :cols]
    body.copy_(t.reshape(rows, cols).to(_dev()))
    return buf, body


class _Output:
    """An output [rows, cols] with row pitch ld inside a buffer filled with the payload."""

    def __init__(self, rows, cols, dtype, ld=None):
        import torch
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.itemsize = torch.empty(0, dtype=dtype).element_size()
        self.g = GUARD_BYTES // self.itemsize
        n = self.g + rows * self.ld + self.g
        self.words = torch.full((n * self.itemsize // 4,), PAYLOAD, dtype=torch.int32, device=_dev())
        self.buf = self.words.view(dtype)
        self.body = self.buf[self.g:self.g + rows * self.ld].view(rows, self.ld)[:, :self.cols]

    def ptr(self):
        return self.body.data_ptr()

    def check(self, what):
        import torch
        torch.cuda.synchronize()
        w = self.words.cpu().numpy().reshape(-1, self.itemsize // 4)        # one row of words per element
        inside = np.zeros(w.shape[0], bool)
        idx = self.g + np.arange(self.rows)[:, None] * self.ld + np.arange(self.cols)[None, :]
        inside[idx.ravel()] = True
        guard = w[~inside]
        bad = np.nonzero((guard != np.int32(PAYLOAD)).any(1))[0]
        assert bad.size == 0, "%s: %d guard elements overwritten" % (what, bad.size)
        body = w[idx.ravel()]
        left = int((body == np.int32(PAYLOAD)).all(1).sum())
        assert left == 0, "%s: %d output elements never written" % (what, left)
        return self.body.cpu().numpy().copy()


def _both(case):
    """case(nan) -> dict of host arrays, with NaN and with zero neighbours: bit-identical."""
    a, b = case(True), case(False)
    for k in a:
        assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)), k
    return a


def _model(d, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    return rng.random(d), q * (0.5 + rng.random(d))[:, None], np.sort(rng.random(d) * 3.0 + 0.05)[::-1].copy()


@pytest.fixture(scope="module")
def eng():
    from plda_amd import MPlda
    return MPlda(0)


@pytest.mark.parametrize("din,dout,r", [(7, 7, 63), (129, 129, 1029), (200, 150, 5001), (257, 257, 333), (520, 520, 77)])
def test_transform_rows_dev_guards(eng, din, dout, r):
    import torch
    mean, T, psi = _model(din, din + r)
    T, psi = T[:dout].copy(), psi[:dout].copy()
    eng.set_model(mean, T, psi)
    rng = np.random.default_rng(r)
    x = rng.standard_normal((r, din))
    n = rng.integers(1, 9, r).astype(np.int32)

    def case(nan):
        _, dx = _input(x, nan)
        _, dn = _input(n, nan)
        o1, o2 = _Output(r, dout, torch.float64), _Output(r, dout, torch.float64)
        torch.cuda.synchronize()
        eng.transform_rows_dev(dx.data_ptr(), r, din, None, 3, o1.ptr())
        eng.transform_rows_dev(dx.data_ptr(), r, din, dn.data_ptr(), 0, o2.ptr())
        eng.synchronize()
        return dict(u=o1.check("uniform"), m=o2.check("per-row counts"))

    a = _both(case)
    # the rule of tests/transform_model.py against the longdouble definition of TransformIvector, never looser than the flat band
    # rtol = 1e-11, atol = 1e-12 these outputs were held to against the NumPy restatement of the device's formula
    import transform_model as TM
    TM.assert_rule_many(a["u"], T, mean, psi, x, 3, "uniform", no_looser_than=(1e-11, 1e-12))
    TM.assert_rule_many(a["m"], T, mean, psi, x, n, "per-row counts", no_looser_than=(1e-11, 1e-12))


@pytest.mark.parametrize("d,m,nt,ld,mixed,znorm", [(51, 333, 517, 530, False, False), (51, 333, 517, 517, True, True),
                                                   (130, 1001, 2003, 2011, True, False), (63, 4099, 4355, 4360, False, True)])
def test_score_matrix_dev_guards(eng, oracle, d, m, nt, ld, mixed, znorm):
    import torch
    from conftest import score_tol
    mean, T, psi = _model(d, d + nt)
    eng.set_model(mean, T, psi)
    rng = np.random.default_rng(m)
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    n = rng.integers(1, 7, m).astype(np.int32) if mixed else np.full(m, 2, np.int32)
    zm, zs = rng.standard_normal(m), rng.random(m) + 0.5

    def case(nan):
        _, dU = _input(U, nan)
        _, dV = _input(V, nan)
        _, dn = _input(n, nan)
        _, dzm = _input(zm, nan)
        _, dzs = _input(zs, nan)
        o = _Output(m, nt, torch.float32, ld)
        torch.cuda.synchronize()
        eng.score_matrix_dev(dU.data_ptr(), dn.data_ptr() if mixed else None, 0 if mixed else 2, m, dV.data_ptr(), nt, o.ptr(), ld,
                             dzm.data_ptr() if znorm else None, dzs.data_ptr() if znorm else None)
        eng.synchronize()
        return dict(S=o.check("scores"))

    a = _both(case)
    ref = oracle.score_block(psi, U, n, V, zm if znorm else None, zs if znorm else None)
    assert (np.abs(a["S"] - ref) <= score_tol(ref)).all()


@pytest.mark.parametrize("d,nb,m", [(48, 391, 40), (207, 600, 5), (230, 520, 7)])
def test_znorm_stats_dev_guards(eng, oracle, d, nb, m):
    import torch
    mean, T, psi = _model(d, d * nb)
    eng.set_model(mean, T, psi)
    model = dict(mean=mean, transform=T, psi=psi, offset=-T @ mean)
    rng = np.random.default_rng(d)
    bkg = rng.random((nb, d))
    models = np.stack([oracle.transform_ivector(model, r, 1) for r in rng.random((m, d)) + 0.1])

    def case(nan):
        _, db = _input(bkg, nan)
        _, dm = _input(models, nan)
        om, os_ = _Output(1, m, torch.float64), _Output(1, m, torch.float64)
        torch.cuda.synchronize()
        eng.znorm_stats_dev(db.data_ptr(), nb, 0, d, dm.data_ptr(), m, om.ptr(), os_.ptr())
        eng.synchronize()
        return dict(zm=om.check("z-norm means")[0], zs=os_.check("z-norm stds")[0])

    a = _both(case)
    rm, rs = oracle.norm(model, bkg, models)
    scale = np.maximum(np.abs(rm), np.abs(rm).mean())
    assert (np.abs(a["zm"] - rm) <= 1e-10 * scale).all()
    assert (np.abs(a["zs"] - rs) <= 1e-10 * np.maximum(rs, 1e-3 * scale)).all()


@pytest.mark.parametrize("m,nt,ld", [(3, 5, 7), (257, 1023, 1030), (1003, 1999, 2004)])
def test_eer_and_det_dev_guards(eng, m, nt, ld):
    from oracle import plda_oracle_np as onp
    from plda_amd import eer
    rng = np.random.default_rng(m + nt)
    es, ts = rng.integers(0, 9, m), rng.integers(0, 9, nt)
    tgt = es[:, None] == ts[None, :]
    S = (rng.standard_normal((m, nt)) + 2.0 * tgt).astype(np.float32)

    def case(nan):
        _, dS = _input(S, nan, ld)
        _, des = _input(es.astype(np.int64), nan)
        _, dts = _input(ts.astype(np.int64), nan)
        out = eer.eer_from_matrix_dev(eng, dS.data_ptr(), ld, m, nt, des.data_ptr(), dts.data_ptr())
        thr, far, frr = eer.det_from_matrix_dev(eng, dS.data_ptr(), ld, m, nt, des.data_ptr(), dts.data_ptr(), 40)
        return dict(e=np.asarray(out, np.float64), thr=thr, far=far, frr=frr)

    a = _both(case)
    ref = onp.eer(S[~tgt], S[tgt])
    assert tuple(a["e"][1:4]) == ref[1:] and a["e"][0] == pytest.approx(ref[0], rel=1e-12)


def test_score_eer_dev_guards(eng):
    from plda_amd import eer
    d, m, nt, k = 41, 1003, 1999, 37
    mean, T, psi = _model(d, 77)
    eng.set_model(mean, T, psi)
    rng = np.random.default_rng(9)
    es, ts = rng.integers(0, k, m), rng.integers(0, k, nt)
    spk = rng.standard_normal((k, d)) * 1.2
    U, V = spk[es] + rng.standard_normal((m, d)), spk[ts] + rng.standard_normal((nt, d))
    n = rng.integers(1, 5, m).astype(np.int32)

    def case(nan):
        _, dU = _input(U, nan)
        _, dV = _input(V, nan)
        _, dn = _input(n, nan)
        _, des = _input(es.astype(np.int64), nan)
        _, dts = _input(ts.astype(np.int64), nan)
        return dict(e=np.asarray(eer.eer_from_operands_dev(eng, dU.data_ptr(), dn.data_ptr(), 0, m, dV.data_ptr(), nt,
                                                           des.data_ptr(), dts.data_ptr()), np.float64))

    a = _both(case)
    # the same EER from the scores of the whole matrix, taken on the host (the matrix form's test holds that to the oracle)
    import torch
    from oracle import plda_oracle_np as onp
    S = torch.empty((m, nt), dtype=torch.float32, device=_dev())
    dU, dV, dn = (torch.from_numpy(v).to(_dev()) for v in (U, V, n))
    torch.cuda.synchronize()
    eng.score_matrix_dev(dU.data_ptr(), dn.data_ptr(), 0, m, dV.data_ptr(), nt, S.data_ptr(), nt)
    eng.synchronize()
    Sh = S.cpu().numpy()
    tgt = es[:, None] == ts[None, :]
    ref = onp.eer(Sh[~tgt], Sh[tgt])
    assert tuple(a["e"][1:4]) == ref[1:] and a["e"][0] == pytest.approx(ref[0], rel=1e-12)
    assert a["e"][4] == tgt.sum() and a["e"][5] == (~tgt).sum()


@pytest.mark.parametrize("d", [33, 200])
def test_fit_dev_guards(eng, d):
    import torch
    from oracle import plda_oracle_np as onp
    x, y = make_data(5 + d, 700, d, 41, skew=True, scale_between=0.5)
    _, dense = np.unique(y, return_inverse=True)
    K = int(dense.max()) + 1

    def case(nan):
        _, dx = _input(x, nan)
        _, dl = _input(dense.astype(np.int64), nan)
        torch.cuda.synchronize()
        eng.fit_dev(dx.data_ptr(), x.shape[0], d, dl.data_ptr(), K, 4)
        eng.synchronize()
        g = eng.get_model()
        means = _Output(K, d, torch.float64)
        counts = _Output(1, K, torch.int64)
        scatter = _Output(d, d, torch.float64)
        eng.fit_get_stats_dev(means.ptr(), counts.ptr(), scatter.ptr())
        eng.synchronize()
        return dict(psi=g["psi"], transform=g["transform"], means=means.check("means"), counts=counts.check("counts"),
                    scatter=scatter.check("scatter"))

    a = _both(case)
    ref = onp.fit(x, dense, 4)
    assert np.abs(a["psi"] - ref["psi"]).max() <= 1e-9 * ref["psi"].max()
    st = onp.stats(x, dense)
    np.testing.assert_array_equal(a["counts"][0], st["counts"])
    assert np.abs(a["means"] - st["means"]).max() < 1e-12
    assert np.abs(a["scatter"] - st["scatter"]).max() <= 1e-12 * np.abs(st["scatter"]).max()


@pytest.mark.parametrize("solver", ["svd", "eigen", "lsqr"])
def test_lda_dev_guards(eng, solver):
    import torch
    from oracle import lda_oracle_np as lo
    from plda_amd.lda import LDA
    x, y = make_data(31, 1500, 45, 23, skew=True, scale_between=0.8)
    _, dense = np.unique(y, return_inverse=True)
    K = int(dense.max()) + 1
    ref = lo.fit(x, dense, solver)

    def case(nan):
        lda = LDA(solver, engine=eng)
        _, dx = _input(x, nan)
        _, dl = _input(dense.astype(np.int64), nan)
        torch.cuda.synchronize()
        lda.fit_dev(dx.data_ptr(), x.shape[0], x.shape[1], dl.data_ptr(), K)
        o = _Output(301, K, torch.float64)
        lda.predict_dev(dx.data_ptr(), 301, 1, o.ptr())
        eng.synchronize()
        return dict(lp=o.check("log-proba"))

    a = _both(case)
    assert np.abs(a["lp"] - lo.predict_log_proba(ref, x[:301])).max() < 1e-8


@pytest.mark.parametrize("d", [33, 200])
def test_fit_stats_em_and_sharded_fit_dev_guards(eng, d):
    """plda_fit_stats_dev -> plda_fit_get_stats_dev (outputs in guarded buffers) -> plda_fit_em_dev reading those statistics
    with NaN neighbours; plda_fit_sharded_dev on one rank."""
    import torch
    from oracle import plda_oracle_np as onp
    x, y = make_data(17 + d, 700, d, 41, skew=True, scale_between=0.5)
    _, dense = np.unique(y, return_inverse=True)
    K = int(dense.max()) + 1

    def case(nan):
        _, dx = _input(x, nan)
        _, dl = _input(dense.astype(np.int64), nan)
        torch.cuda.synchronize()
        eng.fit_stats_dev(dx.data_ptr(), x.shape[0], d, dl.data_ptr(), K)
        means, counts, scatter = _Output(K, d, torch.float64), _Output(1, K, torch.int64), _Output(d, d, torch.float64)
        eng.fit_get_stats_dev(means.ptr(), counts.ptr(), scatter.ptr())
        eng.synchronize()
        st = dict(means=means.check("means"), counts=counts.check("counts"), scatter=scatter.check("scatter"))
        _, dm = _input(st["means"], nan)
        _, dc = _input(st["counts"][0], nan)
        _, ds = _input(st["scatter"], nan)
        torch.cuda.synchronize()
        eng.fit_em_dev(dm.data_ptr(), dc.data_ptr(), K, ds.data_ptr(), d, 4)
        g = eng.get_model()
        eng.fit_sharded_dev(dx.data_ptr(), x.shape[0], d, dl.data_ptr(), K, 4)
        g2 = eng.get_model()
        return dict(psi=g["psi"], transform=g["transform"], psi2=g2["psi"], transform2=g2["transform"], **st)

    a = _both(case)
    ref = onp.fit(x, dense, 4)
    st = onp.stats(x, dense)
    np.testing.assert_array_equal(a["counts"][0], st["counts"])
    assert np.abs(a["scatter"] - st["scatter"]).max() <= 1e-12 * np.abs(st["scatter"]).max()
    for k in ("psi", "psi2"):
        assert np.abs(a[k] - ref["psi"]).max() <= 1e-9 * ref["psi"].max()


@pytest.mark.parametrize("mixed", [False, True])
def test_score_prepare_dev_guards(eng, oracle, mixed):
    """A test side packed ahead of time (plda_score_prepare_dev / _counts_dev) from rows with NaN neighbours."""
    import torch
    from conftest import score_tol
    d, m, nt, ld = 61, 301, 1029, 1040
    mean, T, psi = _model(d, 5 + mixed)
    eng.set_model(mean, T, psi)
    rng = np.random.default_rng(40 + mixed)
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    n = rng.integers(1, 6, m).astype(np.int32) if mixed else np.full(m, 3, np.int32)

    def case(nan):
        _, dU = _input(U, nan)
        _, dV = _input(V, nan)
        _, dn = _input(n, nan)
        torch.cuda.synchronize()
        if mixed:
            eng.score_prepare_counts_dev(dV.data_ptr(), nt, [1, 2, 3, 4, 5])
        else:
            eng.score_prepare_dev(dV.data_ptr(), nt, mixed_counts=False, n_uniform=3)
        o = _Output(m, nt, torch.float32, ld)
        eng.score_matrix_dev(dU.data_ptr(), dn.data_ptr() if mixed else None, 0 if mixed else 3, m, dV.data_ptr(), nt, o.ptr(), ld)
        eng.synchronize()
        out = dict(S=o.check("scores"))
        eng.score_unprepare()
        return out

    a = _both(case)
    ref = oracle.score_block(psi, U, n, V)
    assert (np.abs(a["S"] - ref) <= score_tol(ref)).all()


def test_sharded_entry_points_on_one_rank_guards(eng, oracle):
    """The row-sharded scoring forms and the sharded z-norm statistics on one rank (no communicator): in place with a
    padded leading dimension, compact, and the assembled copy."""
    import torch
    from conftest import score_tol
    d, m, nt, ld, nb = 47, 1000, 777, 790, 333
    mean, T, psi = _model(d, 99)
    eng.set_model(mean, T, psi)
    model = dict(mean=mean, transform=T, psi=psi, offset=-T @ mean)
    rng = np.random.default_rng(99)
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    n = rng.integers(1, 4, m).astype(np.int32)
    bkg = rng.random((nb, d))

    def case(nan):
        _, dU = _input(U, nan)
        _, dV = _input(V, nan)
        _, dn = _input(n, nan)
        _, db = _input(bkg, nan)
        o1 = _Output(m, nt, torch.float32, ld)
        o2, o3 = _Output(m, nt, torch.float32, ld), _Output(m, nt, torch.float32, ld + 3)
        zm, zs = _Output(1, m, torch.float64), _Output(1, m, torch.float64)
        torch.cuda.synchronize()
        eng.score_matrix_sharded_dev(dU.data_ptr(), dn.data_ptr(), 0, m, dV.data_ptr(), nt, o1.ptr(), ld, block_rows=256)
        eng.score_matrix_sharded_local_dev(dU.data_ptr(), dn.data_ptr(), 0, m, dV.data_ptr(), nt, o2.ptr(), ld, block_rows=256,
                                           dfull=o3.ptr(), ld_full=ld + 3)
        eng.znorm_stats_sharded_dev(db.data_ptr(), nb, 0, d, dU.data_ptr(), m, zm.ptr(), zs.ptr())
        eng.synchronize()
        return dict(S1=o1.check("sharded"), S2=o2.check("local"), S3=o3.check("assembled"), zm=zm.check("zmean")[0],
                    zs=zs.check("zstd")[0])

    a = _both(case)
    ref = oracle.score_block(psi, U, n, V)
    for k in ("S1", "S2", "S3"):
        assert (np.abs(a[k] - ref) <= score_tol(ref)).all(), k
    rm, rs = oracle.norm(model, bkg, U)
    scale = np.maximum(np.abs(rm), np.abs(rm).mean())
    assert (np.abs(a["zm"] - rm) <= 1e-10 * scale).all()
    assert (np.abs(a["zs"] - rs) <= 1e-10 * np.maximum(rs, 1e-3 * scale)).all()
