"""GPU: every family of entry points once on fresh device scratch and once on POISONED scratch (PLDA_SCRATCH_POISON=1 at
plda_create: each allocation of the library 64 KiB longer than asked for and filled with 0xFF bytes, NaN as a float -- see
include/plda_hip.h).  Fresh device memory is usually all zero, so a kernel that reads padding, scratch nobody wrote or rows
past the end of a matrix, and multiplies it by zero, is right by luck on fresh memory; on poisoned memory the NaN comes
through.  The two runs must be BIT-identical and the clean run must match the oracle at the tolerances of the family's own
tests.  Also the leak test: create -> the whole pipeline -> destroy, ten times, gives back every byte."""
import os
import tempfile

import numpy as np
import pytest

from conftest import make_data, score_tol
from history_cases import gemm_f64_case, spd_inverse_case, sym_eig_case      # (shared with tests/test_gpu_handle_history.py)

pytestmark = pytest.mark.gpu


def _engine(monkeypatch, poison, env):
    from plda_amd import MPlda
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if poison:
        monkeypatch.setenv("PLDA_SCRATCH_POISON", "1")
    else:
        monkeypatch.delenv("PLDA_SCRATCH_POISON", raising=False)
    eng = MPlda(0)
    for k in list(env) + ["PLDA_SCRATCH_POISON"]:
        monkeypatch.delenv(k, raising=False)
    return eng


def _twice(monkeypatch, case, env=None, exact=True):
    """case(engine) -> dict of arrays, on a fresh handle without and then with the poison switch (a process-wide flag taken
    at every plda_create, so each run is whole before the next handle exists).  Returns the clean run's outputs."""
    from plda_amd import MPlda
    env = env or {}
    out = {}
    for poison in (False, True):
        eng = _engine(monkeypatch, poison, env)
        try:
            out[poison] = {k: np.asarray(v).copy() for k, v in case(eng).items()}
        except Exception as e:
            raise AssertionError("%s scratch: %s" % ("poisoned" if poison else "fresh", e)) from e
        eng.synchronize()
        del eng
    MPlda(0)                       # the switch off again for whatever runs next in this process
    if exact:
        for k, a in out[False].items():
            b = out[True][k]
            assert a.shape == b.shape and a.dtype == b.dtype, k
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), \
                "%s differs on poisoned scratch (%d of %d elements; NaN on poisoned: %d)" % (
                    k, int((a != b).sum()), a.size, int(np.isnan(b).sum()) if b.dtype.kind == "f" else -1)
    return out[False], out[True]


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _model(d, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    return rng.random(d), q * (0.5 + rng.random(d))[:, None], np.sort(rng.random(d) * 3.0 + 0.05)[::-1].copy()


# ---------------------------------------------------------------------------------------------------------------- fit
_FIT_REF = {}


def _fit_ref(d):
    from oracle import plda_oracle_np as onp
    if d not in _FIT_REF:
        x, y = make_data(4000 + d, max(700, 2 * d + 200), d, 41, skew=True, scale_between=0.5)
        _, dense = np.unique(y, return_inverse=True)
        _FIT_REF[d] = (x, y, onp.fit(x, dense, 4, return_wb=True))
    return _FIT_REF[d]


# (forms 1 and 3 skip 209 / 300: the block scatter kernel is the row form's and the default's)
_FIT_CASES = [(f, d) for f in ("0", "1", "3", "4") for d in (1, 17, 33, 200, 209, 257, 300, 511, 512, 700, 1025)
              if not (f in ("1", "3") and d in (209, 300))]


@pytest.mark.parametrize("form,d", _FIT_CASES)
def test_fit_on_poisoned_scratch(monkeypatch, form, d):
    """The four EM forms (PLDA_EM_VARIANT 0 = by shape, 1 = diagonalised basis, 3 = moments, 4 = rows) on 41 speakers with
    skewed counts (19 distinct counts: the row form's G >= 4).  K D = 41 D is odd for odd D: the row form's int4 tile table
    shares one carved buffer with three K x D double arrays (fit.hip: em_rows).  D not a multiple of 16: the row form's fragment loads run past the
    last row of B, X_g and T_g^T.  D in {209, 300, 512}: the block scatter kernel of the rank-k sums.  Form 1 diagonalises
    W = B = I in its first iteration: the direct eigensolver's reflectors of columns that are already tridiagonal (once
    left unwritten) and, at D = 1025, a cold start on every iteration (block Jacobi stops at 1024)."""
    x, y, ref = _fit_ref(d)

    def case(eng):
        eng.fit(x, y, 4)
        it, g = eng.fit_internals(), eng.get_model()
        return dict(W=it["W"], B=it["B"], psi=g["psi"], transform=g["transform"], plan=np.array([eng.fit_plan()["groups"]]))

    a, _ = _twice(monkeypatch, case, {"PLDA_EM_VARIANT": form})
    if form == "4":
        assert a["plan"][0] >= 4
    assert np.abs(a["psi"] - ref["psi"]).max() <= 1e-9 * ref["psi"].max()
    assert _rel(a["W"], ref["W"]) < 1e-9 and _rel(a["B"], ref["B"]) < 1e-9
    assert _rel(a["transform"].T @ a["transform"], ref["transform"].T @ ref["transform"]) < 1e-9


# ---------------------------------------------------------------------------------------------------------- transform
@pytest.mark.parametrize("din,dout", [(7, 7), (77, 77), (129, 129), (200, 150), (209, 209), (257, 257), (385, 385),
                                      (512, 200), (520, 520)])
def test_transform_rows_on_poisoned_scratch(monkeypatch, din, dout):
    from oracle import plda_oracle_np as onp
    mean, T, psi = _model(din, din * 7 + dout)
    T = T[:dout]
    psi = psi[:dout]
    rng = np.random.default_rng(din)
    x = rng.standard_normal((1029, din))
    n = rng.integers(1, 9, 1029).astype(np.int32)

    def case(eng):
        eng.set_model(mean, T, psi)
        return dict(u=eng.transform_array(x, 3), m=eng.transform_array(x, n))

    a, _ = _twice(monkeypatch, case)
    model = dict(mean=mean, transform=T, psi=psi, offset=-T @ mean)
    np.testing.assert_allclose(a["u"], onp.transform_ivector(model, x, 3), rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(a["m"], onp.transform_ivector(model, x, n), rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("d", [37, 200, 230])
def test_transform_groups_and_norm_on_poisoned_scratch(monkeypatch, oracle, d):
    """transform (per-speaker means, TransformIvector) and norm() on the oracle's model (the eigenvectors' signs are free
    between two fits) -- D <= 208: the model pass on the transform kernel's shape with the padded covariance (zn_cpad);
    D > 208: the general GEMM + row kernel."""
    x, y = make_data(60 + d, 900, d, 30, scale_between=0.5)
    ref = oracle.fit(x, y, 4)
    rng = np.random.default_rng(d)
    bkg = rng.random((301, d))
    models = np.stack([oracle.transform_ivector(ref, r, 1) for r in rng.random((13, d)) + 0.1])

    def case(eng):
        eng.set_model(ref["mean"], ref["transform"], ref["psi"])
        tr = eng.transform(x[:400], y[:400])
        eng.norm(bkg, {k: (1, models[k]) for k in range(13)})
        zm, zs = eng.znorm_stats()
        keys = sorted(tr)
        return dict(tv=np.stack([tr[k][1] for k in keys]), tc=np.array([tr[k][0] for k in keys]),
                    zm=np.array([zm[k] for k in range(13)]), zs=np.array([zs[k] for k in range(13)]))

    a, _ = _twice(monkeypatch, case)
    _, rc, rv = oracle.transform_groups(ref, x[:400], y[:400])
    np.testing.assert_array_equal(a["tc"], rc)
    assert np.abs(a["tv"] - rv).max() <= 1e-8 * np.abs(rv).max()
    rm, rs = oracle.norm(ref, bkg, models)
    scale = np.maximum(np.abs(rm), np.abs(rm).mean())
    assert (np.abs(a["zm"] - rm) <= 1e-8 * scale).all()
    assert (np.abs(a["zs"] - rs) <= 1e-8 * np.maximum(rs, 1e-3 * scale)).all()


# -------------------------------------------------------------------------------------------------------------- score
SCORE_ENV_KERNEL = {("PLDA_GEMM_VARIANT", "20"): "trials_gemm_kernel", ("PLDA_GEMM_VARIANT", "40"): "trials_gemm_bt4_kernel",
                    ("PLDA_MIXED_VARIANT", "1"): "trials_gemm_kernel", ("PLDA_SCORE_DTYPE", "bf16x3"): "trials_gemm_bf16x3_kernel"}


@pytest.mark.parametrize("d,m,nt,counts,znorm,env", [
    (51, 333, 517, "uniform", False, {}),
    (51, 333, 517, "mixed", True, {}),
    (130, 1001, 2003, "uniform", True, {}),
    (130, 1001, 2003, "mixed", False, {}),
    (63, 4099, 4355, "uniform", False, {}),                             # large enough for the one-wave-per-SIMD tiles
    (63, 4099, 4355, "mixed", True, {}),
    (94, 700, 1299, "mixed", True, {"PLDA_GEMM_VARIANT": "20"}),
    (94, 700, 1299, "mixed", False, {"PLDA_GEMM_VARIANT": "40"}),
    (94, 700, 1299, "mixed", True, {"PLDA_MIXED_VARIANT": "1"}),
    (77, 1001, 2003, "uniform", True, {"PLDA_SCORE_DTYPE": "bf16x3"}),
    (77, 1001, 2003, "mixed", False, {"PLDA_SCORE_DTYPE": "bf16x3"}),
])
def test_score_matrix_on_poisoned_scratch(monkeypatch, oracle, d, m, nt, counts, znorm, env):
    """The trials GEMM on device operands: M and Nt not multiples of 16 or 256, D not a multiple of 4, uniform and mixed
    enrol counts (the bucketed form by shape and under the forcing arms PLDA_GEMM_VARIANT 20 / 40, and the depth-2D arm
    PLDA_MIXED_VARIANT=1), z-normalised or not, fp32 and bf16x3.  A case that sets a switch also asserts the kernel that ran,
    so that it cannot test something other than its name: at d = 94 with six distinct counts the bucketed depth is 104 (13
    steps of 8 k, 4 stages >= 3), so arm 40 does run the one-wave-per-SIMD kernel at 700 x 1299; 3 x 6 tiles of 256 x 256 are
    the 128 x 128 kernel's by shape."""
    import torch
    dev = torch.device("cuda", 0)
    mean, T, psi = _model(d, d + m)
    rng = np.random.default_rng(m + nt)
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    n = rng.integers(1, 7, m).astype(np.int32) if counts == "mixed" else np.full(m, 3, np.int32)
    zm, zs = rng.standard_normal(m) * 3.0, rng.random(m) * 2.0 + 0.5

    def case(eng):
        eng.set_model(mean, T, psi)
        dU, dV = torch.from_numpy(U).to(dev), torch.from_numpy(V).to(dev)
        dn = torch.from_numpy(n).to(dev)
        dzm, dzs = torch.from_numpy(zm).to(dev), torch.from_numpy(zs).to(dev)
        S = torch.empty((m, nt), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        eng.score_matrix_dev(dU.data_ptr(), dn.data_ptr() if counts == "mixed" else None, 0 if counts == "mixed" else 3, m,
                             dV.data_ptr(), nt, S.data_ptr(), nt, dzm.data_ptr() if znorm else None, dzs.data_ptr() if znorm else None)
        eng.synchronize()
        if env:
            assert eng.score_last_kernel() == SCORE_ENV_KERNEL[next(iter(env.items()))]
        return dict(S=S.cpu().numpy())

    a, _ = _twice(monkeypatch, case, env)
    ref = oracle.score_block(psi, U, n, V, zm if znorm else None, zs if znorm else None)
    tol = score_tol(ref) * (10.0 if env.get("PLDA_SCORE_DTYPE") == "bf16x3" else 1.0)
    assert (np.abs(a["S"] - ref) <= tol).all(), np.abs(a["S"] - ref).max()


def test_score_pairs_on_poisoned_scratch(monkeypatch, oracle):
    d, m, nt, p = 45, 57, 91, 20011
    mean, T, psi = _model(d, 5)
    rng = np.random.default_rng(8)
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    n = rng.integers(1, 5, m).astype(np.int32)
    e, t = rng.integers(0, m, p), rng.integers(0, nt, p)

    def case(eng):
        eng.set_model(mean, T, psi)
        return dict(s=eng.score_trials((n, U), (1, V), e, t, znorm=False))

    a, _ = _twice(monkeypatch, case)
    ref = oracle.score_block(psi, U, n, V)[e, t]
    assert (np.abs(a["s"] - ref) <= score_tol(ref)).all()


@pytest.mark.parametrize("d,nb", [(48, 391), (207, 600), (230, 520)])
@pytest.mark.parametrize("variant", ["0", "1", "2", "3"])
def test_znorm_statistics_on_poisoned_scratch(monkeypatch, oracle, d, nb, variant):
    """The four z-norm statistics arms.  Arm 1 sums its column statistics with floating-point atomics (score.hip), whose
    order varies from run to run: it is held to the oracle only, not to bit identity."""
    mean, T, psi = _model(d, d * 3 + nb)
    model = dict(mean=mean, transform=T, psi=psi, offset=-T @ mean)
    rng = np.random.default_rng(d + nb)
    bkg = rng.random((nb, d))
    models = np.stack([oracle.transform_ivector(model, r, 1) for r in rng.random((9, d)) + 0.1])

    def case(eng):
        eng.set_model(mean, T, psi)
        eng.norm(bkg, {k: (1, models[k]) for k in range(9)})
        zm, zs = eng.znorm_stats()
        return dict(zm=np.array([zm[k] for k in range(9)]), zs=np.array([zs[k] for k in range(9)]))

    a, b = _twice(monkeypatch, case, {"PLDA_ZNORM_VARIANT": variant}, exact=variant != "1")
    rm, rs = oracle.norm(model, bkg, models)
    tol = 1e-10 if variant != "1" else 1e-4
    scale = np.maximum(np.abs(rm), np.abs(rm).mean())
    for r in (a, b):
        assert (np.abs(r["zm"] - rm) <= tol * scale).all()
        assert (np.abs(r["zs"] - rs) <= tol * np.maximum(rs, 1e-3 * scale)).all()


# ------------------------------------------------------------------------------------------------------ around the path
@pytest.mark.parametrize("variant", ["1", "2"])
def test_eer_and_det_on_poisoned_scratch(monkeypatch, variant):
    """plda_eer_matrix_dev in the three-pass (1) and the single-pass (2) form, plda_score_eer_dev, DET points."""
    import torch
    from oracle import plda_oracle_np as onp
    from plda_amd import eer
    dev = torch.device("cuda", 0)
    d, m, nt, k = 41, 1003, 1999, 37
    mean, T, psi = _model(d, 77)
    rng = np.random.default_rng(9)
    es, ts = rng.integers(0, k, m), rng.integers(0, k, nt)
    spk = rng.standard_normal((k, d)) * 1.2
    U, V = spk[es] + rng.standard_normal((m, d)), spk[ts] + rng.standard_normal((nt, d))

    def case(eng):
        eng.set_model(mean, T, psi)
        dU, dV = torch.from_numpy(U).to(dev), torch.from_numpy(V).to(dev)
        des, dts = torch.from_numpy(es).to(dev), torch.from_numpy(ts).to(dev)
        S = torch.empty((m, nt + 5), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        eng.score_matrix_dev(dU.data_ptr(), None, 1, m, dV.data_ptr(), nt, S.data_ptr(), nt + 5)
        eng.synchronize()
        a = eer.eer_from_matrix_dev(eng, S.data_ptr(), nt + 5, m, nt, des.data_ptr(), dts.data_ptr())
        b = eer.eer_from_operands_dev(eng, dU.data_ptr(), None, 1, m, dV.data_ptr(), nt, des.data_ptr(), dts.data_ptr())
        thr, far, frr = eer.det_from_matrix_dev(eng, S.data_ptr(), nt + 5, m, nt, des.data_ptr(), dts.data_ptr(), 50)
        return dict(S=S[:, :nt].cpu().numpy(), a=np.asarray(a, np.float64), b=np.asarray(b, np.float64), thr=thr, far=far, frr=frr)

    r, _ = _twice(monkeypatch, case, {"PLDA_EER_VARIANT": variant})
    tgt = es[:, None] == ts[None, :]
    ref = onp.eer(r["S"][~tgt], r["S"][tgt])
    assert tuple(r["a"][1:4]) == ref[1:] and r["a"][0] == pytest.approx(ref[0], rel=1e-12)
    assert np.array_equal(r["a"], r["b"])
    thr, far, frr = onp.det(r["S"][~tgt], r["S"][tgt], 50)
    assert np.array_equal(r["thr"], thr) and np.array_equal(r["far"], far) and np.array_equal(r["frr"], frr)


@pytest.mark.parametrize("solver", ["svd", "eigen", "lsqr"])
def test_lda_on_poisoned_scratch(monkeypatch, solver):
    from oracle import lda_oracle_np as lo
    from plda_amd.lda import LDA
    x, y = make_data(31, 1500, 45, 23, skew=True, scale_between=0.8)

    def case(eng):
        lda = LDA(solver, engine=eng)
        lda.fit(x, y)
        return dict(lp=lda.predict_log_proba(x[:301]), tr=lda.transform(x[:301]) if solver != "lsqr" else np.zeros(1))

    a, _ = _twice(monkeypatch, case)
    ref = lo.fit(x, y, solver)
    assert np.abs(a["lp"] - lo.predict_log_proba(ref, x[:301])).max() < 1e-8


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("method", ["mean", "max", "var"])
def test_dvector_pool_on_poisoned_scratch(monkeypatch, dtype, method):
    """D % 4 != 0: the scalar kernel, not the vec4 one."""
    from oracle import plda_oracle_np as onp
    from plda_amd import dvector
    rng = np.random.default_rng(3)
    frames = rng.standard_normal((5003, 203)).astype(dtype)
    offsets = np.concatenate([[0], np.sort(rng.choice(np.arange(1, 5003), 40, replace=False)), [5003]])

    def case(eng):
        return dict(p=dvector.pool(frames, offsets, method, True, engine=eng))

    a, _ = _twice(monkeypatch, case)
    ref = onp.dvector_pool(frames.astype(np.float64), offsets, method, True)
    np.testing.assert_allclose(a["p"], ref, rtol=1e-9 if dtype == np.float64 else 1e-5, atol=1e-9)


def test_htk_frames_on_poisoned_scratch(monkeypatch):
    from oracle import htk_oracle_np as ho
    from plda_amd import htk
    rng = np.random.default_rng(4)
    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for i, (t, d) in enumerate([(37, 23), (1, 23), (211, 23)]):
            f = os.path.join(tmp, "%d.htk" % i)
            ho.write_htk(f, rng.standard_normal((t, d)).astype(np.float32))
            files.append(f)

        def case(eng):
            return {str(i): htk.htk_load(f, 2, engine=eng).view(np.uint32) for i, f in enumerate(files)}

        a, _ = _twice(monkeypatch, case)
        for i, f in enumerate(files):
            assert np.array_equal(a[str(i)], ho.htk_load(open(f, "rb").read(), 2))


@pytest.mark.parametrize("n", [7, 65, 200, 333])
def test_sym_eig_on_poisoned_scratch(monkeypatch, n):
    """Default, block Jacobi and the direct method (tridiagonalisation + divide and conquer)."""
    rng = np.random.default_rng(n)
    A = rng.standard_normal((n, n))
    G = A @ A.T / n + np.diag(rng.random(n))
    lam_ref = np.sort(np.linalg.eigvalsh(G))[::-1]
    a, _ = _twice(monkeypatch, sym_eig_case(G))
    for method in (0, 1, 2):
        lam, V = a["lam%d" % method], a["V%d" % method]
        assert np.abs(lam - lam_ref).max() < 1e-11 * lam_ref.max()
        assert np.abs((V * lam[:, None]).T @ V - G).max() < 1e-10 * np.abs(G).max()


@pytest.mark.parametrize("n", [3, 16, 17, 31, 32, 33, 100])
def test_sym_eig_of_diagonal_input_on_poisoned_scratch(monkeypatch, n):
    """Input that is already diagonal (the basis-form EM's first iteration diagonalises I): every column needs no
    reflection, and the back-transformation must still read a zero reflector, not whatever the scratch held."""
    Gs = [np.eye(n), np.diag(np.arange(1.0, n + 1.0))]

    def case(eng):
        out = {}
        for i, G in enumerate(Gs):
            for method in (0, 2):
                lam, V, used = eng.sym_eig(G, method)
                out["lam%d%d" % (i, method)], out["V%d%d" % (i, method)] = lam, V
        return out

    a, _ = _twice(monkeypatch, case)
    for i, G in enumerate(Gs):
        for method in (0, 2):
            lam, V = a["lam%d%d" % (i, method)], a["V%d%d" % (i, method)]
            assert np.array_equal(lam, np.sort(np.diag(G))[::-1])
            assert np.abs(V @ V.T - np.eye(n)).max() < 1e-14
            assert np.abs((V * lam[:, None]).T @ V - G).max() < 1e-14


@pytest.mark.parametrize("d", [1, 16, 17, 33, 65, 128, 200, 209, 256, 257, 300, 512])
def test_spd_inverse_on_poisoned_scratch(monkeypatch, d):
    rng = np.random.default_rng(d)
    A = rng.standard_normal((d, d + 5))
    A = A @ A.T + 0.5 * np.eye(d)
    a, _ = _twice(monkeypatch, spd_inverse_case(A))
    assert np.abs(a["x"] @ A - np.eye(d)).max() < 1e-9


@pytest.mark.parametrize("m,n,k,batch", [(1, 1, 1, 1), (17, 33, 9, 1), (200, 200, 200, 3), (257, 130, 1031, 1), (64, 64, 20000, 1)])
def test_gemm_f64_on_poisoned_scratch(monkeypatch, m, n, k, batch):
    rng = np.random.default_rng(m + n + k)
    A = rng.standard_normal((batch, m, k)) if batch > 1 else rng.standard_normal((k, m))
    B = rng.standard_normal((batch, k, n)) if batch > 1 else rng.standard_normal((k, n))
    w = rng.random(k)
    Cin = rng.standard_normal((batch, m, n) if batch > 1 else (m, n))
    a, _ = _twice(monkeypatch, gemm_f64_case(A, B, w, Cin, batch))
    ref = 0.5 * (A @ B) + 2.0 * Cin if batch > 1 else 0.5 * (A.T * w) @ B + 2.0 * Cin
    assert np.abs(a["c"] - ref).max() < 1e-12 * max(1.0, np.abs(ref).max()) * np.sqrt(k)


def test_poison_switch_refused_while_capturing():
    """A fill that would land inside a graph capture of the handle's stream is an error code, never an abort.  In a child
    process of its own (a capture that ends in an error must not leave state behind for the rest of the suite); relaxed
    capture mode, so that the allocation itself is allowed and the library's own check is what refuses."""
    import subprocess
    import sys
    import textwrap
    from conftest import ROOT
    code = textwrap.dedent("""
        import os
        os.environ["PLDA_SCRATCH_POISON"] = "1"
        import numpy as np, torch
        from plda_amd import MPlda
        from plda_amd._native import PldaError
        dev = torch.device("cuda", 0)
        d, m, nt = 24, 40, 50
        rng = np.random.default_rng(1)
        q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        eng = MPlda(0)
        eng.set_model(rng.random(d), q, np.sort(rng.random(d) + 0.1)[::-1].copy())
        U = torch.randn((m, d), dtype=torch.float64, device=dev)
        V = torch.randn((nt, d), dtype=torch.float64, device=dev)
        S = torch.empty((m, nt), dtype=torch.float32, device=dev)
        s = torch.cuda.Stream(dev)
        torch.cuda.synchronize()
        eng.set_stream(s.cuda_stream)
        g = torch.cuda.CUDAGraph()
        msg = "not refused"
        with torch.cuda.stream(s):
            g.capture_begin(capture_error_mode="relaxed")
            try:
                eng.score_matrix_dev(U.data_ptr(), None, 1, m, V.data_ptr(), nt, S.data_ptr(), nt)
            except PldaError as e:
                msg = "refused: %s" % e
            g.capture_end()
        print(msg)
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "refused" in r.stdout and "captur" in r.stdout, r.stdout[-2000:]


# ---------------------------------------------------------------------------------------------------------------- leak
def test_create_pipeline_destroy_gives_back_every_byte():
    """Ten cycles of create -> fit in both grouped EM forms -> transform -> norm -> score with z-norm -> EER -> LDA fit
    -> destroy: plda_device_bytes_held() back at its first value, to the byte (every DevBuf of a handle is freed by its
    destructor; before that plda_destroy freed a hand-kept list that missed the row-form EM's chunk table and norm()'s padded
    covariance)."""
    import gc
    import torch
    from plda_amd import MPlda, eer
    from plda_amd import _native as N
    from plda_amd.lda import LDA
    lib = N.load()
    dev = torch.device("cuda", 0)
    x, y = make_data(12, 900, 40, 30, skew=True, scale_between=0.5)
    rng = np.random.default_rng(12)
    bkg = rng.random((200, 40))
    gc.collect()
    first = lib.plda_device_bytes_held()
    for cycle in range(10):
        for form in ("3", "4"):
            os.environ["PLDA_EM_VARIANT"] = form
            try:
                eng = MPlda(0)
            finally:
                del os.environ["PLDA_EM_VARIANT"]
            eng.fit(x, y, 3)
            tr = eng.transform(x[:300], y[:300])
            ids = sorted(tr)
            eng.norm(bkg, {k: tr[k] for k in ids})
            U = torch.from_numpy(np.stack([tr[k][1] for k in ids])).to(dev)
            V = torch.from_numpy(eng.transform_array(x[300:700], 1)).to(dev)
            zm, zs = eng.znorm_stats()
            dzm = torch.tensor([zm[k] for k in ids], dtype=torch.float64, device=dev)
            dzs = torch.tensor([zs[k] for k in ids], dtype=torch.float64, device=dev)
            S = torch.empty((len(ids), 400), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            eng.score_matrix_dev(U.data_ptr(), None, 1, len(ids), V.data_ptr(), 400, S.data_ptr(), 400, dzm.data_ptr(), dzs.data_ptr())
            eng.synchronize()
            es = torch.tensor(ids, dtype=torch.int64, device=dev)
            ts = torch.from_numpy(y[300:700].astype(np.int64)).to(dev)
            eer.eer_from_matrix_dev(eng, S.data_ptr(), 400, len(ids), 400, es.data_ptr(), ts.data_ptr())
            LDA("svd", engine=eng).fit(x, y)
            assert lib.plda_device_bytes_held() > first
            del eng
            gc.collect()
        held = lib.plda_device_bytes_held()
        assert held == first, "cycle %d: %d bytes of device memory not given back" % (cycle, held - first)
