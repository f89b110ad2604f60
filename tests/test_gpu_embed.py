"""GPU: the embedding chain (K18; csrc/embed.hip) against its NumPy model (tests/embed_model.py) and its contract
(include/plda_hip.h, "embedding chain"): the a-priori error bound in every dispatch class, bits that do not depend on the
batch, guard bands, poisoned scratch, leaks, every refusal, the three fits, and the raw-row methods of liblda.PLDA."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed_model as em  # noqa: E402
from test_embed_model import FORMS, make_chain  # noqa: E402

pytestmark = pytest.mark.gpu

E_INVAL, E_NUMERIC, E_NOT_FITTED = -1, -3, -4


def _engine(monkeypatch, **env):
    from plda_amd import MPlda
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = MPlda(0)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    return eng


@pytest.fixture(scope="module")
def eng():
    from plda_amd import MPlda
    return MPlda(0)


@pytest.fixture(scope="module")
def engines():
    """default | sized for 2 compute units (every block shape and the main + tail split at a few hundred rows) | class 2 forced."""
    from plda_amd import MPlda
    mp = pytest.MonkeyPatch()
    out = {"default": MPlda(0)}
    mp.setenv("PLDA_EMBED_CUS", "2")
    out["cus2"] = MPlda(0)
    mp.delenv("PLDA_EMBED_CUS")
    mp.setenv("PLDA_EMBED_VARIANT", "1")
    out["forced"] = MPlda(0)
    mp.delenv("PLDA_EMBED_VARIANT")
    mp.undo()
    return out


def _chain(ch):
    from plda_amd.embed import EmbeddingChain
    d = ch.A.shape[1] if ch.A is not None else len(ch.m_in) if ch.m_in is not None else len(ch.m_out)
    return EmbeddingChain(ch.m_in, ch.len_in, ch.A, ch.m_out, ch.len_out, dim=d)


def _plan(e, din, dout, has_a, dtype=0):
    out = np.zeros(3, np.int32)
    e._ck(e._lib.plda_embed_plan(e._h, din, dout, int(has_a), dtype, out.ctypes.data_as(C.c_void_p)))
    return [int(v) for v in out]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _ratio(got, ch, x):
    ref = em.apply(ch, x, np.longdouble)
    bound = em.error_bound(ch, x)
    err = np.abs(np.asarray(got, np.longdouble) - ref).astype(np.float64)
    assert np.all(np.isfinite(got))
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))))


# Din below, at and across the 16-deep stage, C2's size, above 512; Dout at the tile edge and the class-1 / class-2 boundary
# (every class is hit -- 0 by the forms without A, 1 and 2 on either side of Dout = 512 -- and asserted through plda_embed_plan)
PAIRS = [(1, 1), (7, 15), (16, 16), (17, 17), (17, 1), (200, 150), (256, 200), (520, 512), (520, 513)]


@pytest.mark.parametrize("din,dout", PAIRS)
def test_apply_within_the_bound(eng, din, dout):
    rng = np.random.default_rng(din * 7919 + dout)
    worst = 0.0
    for form in FORMS:
        for offset in (0.0, 1e5):
            ch = make_chain(form, din, dout, rng, offset)
            eng.set_embedding(_chain(ch))
            cls = _plan(eng, din, dout if ch.A is not None else din, ch.A is not None)[0]
            assert cls == (0 if ch.A is None else 1 if dout <= 512 else 2)
            for dt in (np.float32, np.float64):
                x = (rng.standard_normal((17, din)) + offset).astype(dt)
                for r in (1, 15, 16, 17):
                    got = eng.embed(x[:r])
                    ratio = _ratio(got, ch, x[:r])
                    worst = max(worst, ratio)
                    print("embed %s din %d dout %d offset %g %s R %d class %d: %.3f of the bound" % (
                        form, din, dout, offset, np.dtype(dt).name, r, cls, ratio))
                    assert ratio <= 1.0, (form, offset, dt, r, ratio)
    eng.set_embedding(None)


# one shape per Dout class of the fused kernel, one of class 0, one of class 2
BIT_SHAPES = [(17, 100, True), (200, 150, True), (256, 250, True), (300, 380, True), (520, 512, True), (200, 200, False), (130, 513, True)]


@pytest.mark.parametrize("din,dout,has_a", BIT_SHAPES)
def test_bits_do_not_depend_on_the_batch(engines, din, dout, has_a):
    rng = np.random.default_rng(din + 31 * dout)
    ch = make_chain("vbx" if has_a else "len_in_only", din, dout, rng)
    if not has_a:
        ch.len_out = 3.0
    x = rng.standard_normal((1000, din)).astype(np.float32)
    e0, e2 = engines["default"], engines["cus2"]
    for e in (e0, e2):
        e.set_embedding(_chain(ch))
    cls, main, _ = _plan(e0, din, dout, has_a, 1)
    full = e0.embed(x)
    assert _ratio(full[:129], ch, x[:129]) <= 1.0
    assert _same(full, e0.embed(x)), "run to run"
    assert _same(full, e0.embed(x.astype(np.float64))), "fp32 against its widened copy"
    for i in (0, 1, 499, 999):
        assert _same(full[i:i + 1], e0.embed(x[i:i + 1])), "row %d alone" % i
    idx = np.array([999, 3, 500, 17, 16, 15, 0, 1, 2, 640, 128, 127, 64, 63, 32, 31, 998])
    assert _same(full[idx], e0.embed(x[idx])), "inside a 17-row batch at other positions"
    # both sides of every block height, a main + tail split, and the whole call, on the handle whose split is sized for 2 CUs
    heights = [h for h in (16, 32, 64, 128) if h <= main] if cls == 1 else [4]
    rs = sorted(set([1, 15, 16, 17, 1000, 2 * main + 44] + [h + s for h in heights for s in (-1, 0, 1) if h + s > 0]))
    for r in rs:
        assert _same(full[:r], e2.embed(x[:r])), "R = %d on the 2-CU split" % r
    assert _same(full[idx], e2.embed(x[idx]))
    for e in (e0, e2):
        e.set_embedding(None)


@pytest.mark.parametrize("din,dout", [(7, 15), (200, 150), (256, 200), (520, 512)])
def test_forced_class_two(engines, din, dout):
    e = engines["forced"]
    rng = np.random.default_rng(din)
    for form in ("kaldi", "vbx", "A_mout"):
        ch = make_chain(form, din, dout, rng, 1e5 if form == "kaldi" else 0.0)
        e.set_embedding(_chain(ch))
        assert _plan(e, din, dout, True)[0] == 2
        x = (rng.standard_normal((40, din)) + (1e5 if form == "kaldi" else 0.0)).astype(np.float32 if form == "vbx" else np.float64)
        got = e.embed(x)
        ratio = _ratio(got, ch, x)
        print("forced class 2 %s %d -> %d: %.3f of the bound" % (form, din, dout, ratio))
        assert ratio <= 1.0
        assert _same(got[7:8], e.embed(x[7:8])) and _same(got[[39, 0, 7]], e.embed(x[[39, 0, 7]]))
    e.set_embedding(None)


@pytest.mark.parametrize("which,din,dout,has_a", [("default", 24, 24, False), ("default", 40, 33, True), ("default", 40, 520, True),
                                                  ("forced", 40, 33, True)])
def test_zero_rows_stay_zero_and_bad_rows_stay_alone(engines, which, din, dout, has_a):
    e = engines[which]
    rng = np.random.default_rng(5)
    m_in = rng.standard_normal(din)
    A = rng.standard_normal((dout, din)) if has_a else None
    x = rng.standard_normal((37, din))
    x[3] = m_in                                       # |v| = 0
    x[20, din // 2] = np.nan
    x[36, 0] = np.inf
    for m_out in (None, rng.standard_normal(dout)):
        ch = em.Chain(m_in, 1.0, A, m_out, 2.0)
        e.set_embedding(_chain(ch))
        out = e.embed(x)
        bad = ~np.all(np.isfinite(out), axis=1)
        assert list(np.nonzero(bad)[0]) == [20, 36]
        if m_out is None:
            assert np.all(out[3] == 0)                # zero at the first norm, zero u, zero at the second
        good = np.array([i for i in range(37) if i not in (20, 36)])
        assert _ratio(out[good], ch, x[good]) <= 1.0
    e.set_embedding(None)


@pytest.mark.parametrize("which,din,dout,has_a", [("default", 130, 130, False), ("default", 130, 150, True), ("cus2", 130, 150, True),
                                                  ("default", 130, 513, True)])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_guard_bands(engines, which, din, dout, has_a, dt):
    import torch
    from test_gpu_guard_bands import _Output, _input
    e = engines[which]
    rng = np.random.default_rng(8)
    ch = make_chain("vbx" if has_a else "len_in_only", din, dout, rng)
    e.set_embedding(_chain(ch))
    r = 301
    x = rng.standard_normal((r, din)).astype(dt)
    res = []
    for nan in (True, False):
        buf, dx = _input(x, nan)
        before = buf.clone()
        o = _Output(r, dout, torch.float64)
        torch.cuda.synchronize()
        e.embed_dev(dx.data_ptr(), 1 if dt == np.float32 else 0, r, din, o.ptr())
        e.synchronize()
        res.append(o.check("embed_apply_dev"))
        assert torch.equal(buf.view(torch.uint8), before.view(torch.uint8)), "X changed"
    assert _same(res[0], res[1]) and _same(res[0], e.embed(x))
    e.set_embedding(None)


def _fit_data(d, rng, offset=0.0, n=None):
    """N = 4 D rows, speakers of 3 ... 12 rows, planted spectra with a gap behind direction dout = min(D // 2 + 1, K - 2) (an
    LDA has K - 1 directions)."""
    n = n or 4 * d
    counts = []
    while sum(counts) < n:
        counts.append(min(int(rng.integers(3, 13)), n - sum(counts)))
    if counts[-1] < 3 and len(counts) > 1:
        last = counts.pop()
        counts[-1] += last
    lab = np.repeat(np.arange(len(counts)), counts).astype(np.uint64)
    dout = max(1, min(d // 2 + 1, len(counts) - 2))
    bstd = np.concatenate([np.linspace(6.0, 4.0, dout), np.linspace(0.5, 0.2, d - dout)])
    wstd = np.linspace(1.0, 1.5, d)
    basis = np.linalg.qr(rng.standard_normal((d, d)))[0]
    x = ((rng.standard_normal((len(counts), d)) * bstd)[lab] + rng.standard_normal((n, d)) * wstd) @ basis + offset
    return x, lab, dout


def _fit_case(e, kind, x, lab, dout, len_in=0.0):
    name = ("centre", "whiten", "lda")[kind]
    ch = e.fit_embedding(x, lab if kind == 2 else None, name, None if kind == 0 else dout, len_in, 1.0)
    return dict(m_in=ch.m_in, A=ch.A if ch.A is not None else np.zeros(0), m_out=ch.m_out, eig=ch.eig if ch.eig is not None else np.zeros(0),
                y=e.embed(x[:50]))


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_poisoned_scratch(monkeypatch, kind):
    from test_gpu_scratch_poison import _twice
    rng = np.random.default_rng(11)
    x, lab, dout = _fit_data(24, rng)
    chains = [make_chain("centre", 24, 24, rng), make_chain("vbx", 24, 13, rng), make_chain("vbx", 24, 520, rng)]
    xs = rng.standard_normal((70, 24)).astype(np.float32)

    def case(e):
        out = _fit_case(e, kind, x, lab, dout)
        for i, ch in enumerate(chains):
            e.set_embedding(_chain(ch))
            out["apply%d" % i] = e.embed(xs)
        return out
    clean, _ = _twice(monkeypatch, case)
    for i, ch in enumerate(chains):
        assert _ratio(clean["apply%d" % i], ch, xs) <= 1.0


def test_no_leak(monkeypatch):
    from plda_amd import MPlda
    lib = MPlda(0)._lib
    rng = np.random.default_rng(12)
    x, lab, dout = _fit_data(24, rng)
    chains = [make_chain("centre", 24, 24, rng), make_chain("vbx", 24, 13, rng), make_chain("vbx", 24, 520, rng)]
    xs = rng.standard_normal((70, 24))
    start = lib.plda_device_bytes_held()
    for _ in range(10):
        e = MPlda(0)
        for ch in chains:
            e.set_embedding(_chain(ch))
            e.embed(xs)
        for kind in (0, 1, 2):
            _fit_case(e, kind, x, lab, dout)
        assert lib.plda_device_bytes_held() > start
        lib.plda_destroy(e._h)
        e._h = None
        assert lib.plda_device_bytes_held() == start


def _get_bytes(e):
    din, dout, fl = C.c_int32(), C.c_int32(), C.c_int32()
    e._ck(e._lib.plda_embed_dims(e._h, C.byref(din), C.byref(dout), C.byref(fl)))
    m_in, A, m_out = np.full(din.value, 7.0), np.full((dout.value, din.value), 7.0), np.full(dout.value, 7.0)
    li, lo = C.c_double(), C.c_double()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    e._ck(e._lib.plda_embed_get(e._h, vp(m_in), C.byref(li), vp(A), vp(m_out), C.byref(lo)))
    return (din.value, dout.value, fl.value, m_in.tobytes(), A.tobytes(), m_out.tobytes(), li.value, lo.value)


def test_every_refusal_leaves_the_chain_and_the_outputs_alone(eng):
    lib, h = eng._lib, eng._h
    rng = np.random.default_rng(13)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    assert lib.plda_embed_clear(h) == 0
    assert lib.plda_embed_dims(h, None, None, None) == E_NOT_FITTED
    x = rng.standard_normal((6, 5))
    out = np.full((6, 3), 9.0)
    assert lib.plda_embed_apply(h, vp(x), 0, 6, 5, vp(out)) == E_NOT_FITTED and np.all(out == 9.0)
    ch = make_chain("vbx", 5, 3, rng)
    eng.set_embedding(_chain(ch))
    kept = _get_bytes(eng)
    assert kept[:3] == (5, 3, 7) and kept[3] == ch.m_in.tobytes() and kept[4] == ch.A.tobytes() and kept[5] == ch.m_out.tobytes()
    m5, m3, a35, big = np.zeros(5), np.zeros(3), np.ones((3, 5)), np.zeros(4097)
    nan5, nana = np.array([0, 0, np.nan, 0, 0.0]), np.full((3, 5), np.inf)
    sets = [(0, 3, None, 0.0, a35, None, 0.0), (4097, 3, big, 0.0, np.ones((3, 4097)), None, 0.0), (5, 0, m5, 0.0, a35, None, 0.0),
            (5, 2049, m5, 0.0, np.ones((2049, 5)), None, 0.0), (5, 3, m5, 0.0, None, None, 0.0), (5, 3, m5, -1.0, a35, m3, 0.0),
            (5, 3, m5, np.nan, a35, m3, 0.0), (5, 3, m5, 0.0, a35, m3, np.inf), (5, 3, m5, 0.0, a35, m3, -0.5), (5, 3, nan5, 0.0, a35, m3, 0.0),
            (5, 3, m5, 0.0, nana, m3, 0.0), (5, 3, m5, 0.0, a35, np.array([0, np.inf, 0.0]), 0.0)]
    for din, dout, mi, li, a, mo, lo in sets:
        assert lib.plda_embed_set(h, din, dout, vp(mi), li, vp(a), vp(mo), lo) == E_INVAL, (din, dout, li, lo)
        assert _get_bytes(eng) == kept
    assert lib.plda_embed_apply(h, vp(x), 0, 6, 4, vp(out)) == E_INVAL          # Din of the call
    assert lib.plda_embed_apply(h, vp(x), 2, 6, 5, vp(out)) == E_INVAL          # dtype
    assert lib.plda_embed_apply_dev(h, None, 0, 6, 4, None) == E_INVAL and lib.plda_embed_apply_dev(h, None, 3, 6, 5, None) == E_INVAL
    assert lib.plda_embed_apply(h, vp(x), 0, 0, 5, vp(out)) == 0                # R = 0: nothing, as plda_transform_rows
    assert np.all(out == 9.0)
    plan = np.full(3, 9, np.int32)
    for args in ((0, 3, 1, 0), (5, 3, 0, 0), (5, 3, 1, 2), (4097, 3, 1, 0), (5, 2049, 1, 0)):
        assert lib.plda_embed_plan(h, *args, vp(plan)) == E_INVAL and np.all(plan == 9)
    xf, lab = rng.standard_normal((12, 5)), np.repeat(np.arange(4), 3).astype(np.uint64)
    eig = np.full(5, 9.0)
    fits = [(xf, 2, 12, 5, lab, 1, 3, 0.0, 1.0), (xf, 0, 12, 5, lab, 3, 3, 0.0, 1.0), (xf, 0, 12, 5, lab, -1, 3, 0.0, 1.0),
            (xf, 0, 12, 5, lab, 1, 6, 0.0, 1.0), (xf, 0, 12, 5, lab, 2, 6, 0.0, 1.0), (xf, 0, 12, 5, lab, 0, 3, 0.0, 1.0),
            (xf, 0, 12, 5, None, 2, 3, 0.0, 1.0), (xf, 0, 1, 5, lab, 1, 3, 0.0, 1.0), (xf, 0, 12, 5, lab, 1, 3, -1.0, 1.0),
            (xf, 0, 12, 5, lab, 1, 3, 0.0, np.nan), (xf, 0, 12, 0, lab, 1, 3, 0.0, 1.0), (xf, 0, 12, 5, np.zeros(12, np.uint64), 2, 3, 0.0, 1.0)]
    for xx, dt, n, din, ll, kind, dout, li, lo in fits:
        assert lib.plda_embed_fit(h, vp(xx), dt, n, din, vp(ll), kind, dout, li, lo, vp(eig)) == E_INVAL, (dt, n, din, kind, dout, li, lo)
        assert _get_bytes(eng) == kept and np.all(eig == 9.0)
    wide, wlab = np.zeros((4, 2049)), np.array([0, 0, 1, 1], np.uint64)
    for kind in (1, 2):                                                                              # the eigensolver's limit
        assert lib.plda_embed_fit(h, vp(wide), 0, 4, 2049, vp(wlab), kind, 3, 0.0, 1.0, vp(eig)) == E_INVAL
        assert _get_bytes(eng) == kept and np.all(eig == 9.0)
    assert lib.plda_embed_fit_dev(h, None, 0, 12, 5, None, 0, 2, 3, 0.0, 1.0, None) == E_INVAL       # kind 2 without labels
    assert lib.plda_embed_fit_dev(h, None, 0, 12, 5, None, 0, 1, 6, 0.0, 1.0, None) == E_INVAL
    # numeric failures: a singular W, fewer directions than Dout -- PLDA_E_NUMERIC, the chain untouched
    xs = xf.copy()
    xs[:, 2] = 1.5
    assert lib.plda_embed_fit(h, vp(xs), 0, 12, 5, vp(lab), 2, 3, 0.0, 1.0, vp(eig)) == E_NUMERIC and _get_bytes(eng) == kept
    xr = rng.standard_normal((12, 2)) @ rng.standard_normal((2, 5))
    assert lib.plda_embed_fit(h, vp(xr), 0, 12, 5, None, 1, 3, 0.0, 1.0, vp(eig)) == E_NUMERIC and _get_bytes(eng) == kept
    got = eng.embed(x)
    assert _ratio(got, ch, x) <= 1.0
    eng.set_embedding(None)


BAND = 1e-8


def _close(a, b, what):
    tol = BAND * float(np.max(np.abs(b)))
    err = float(np.max(np.abs(a - b)))
    print("%s: %.3g (band %.3g)" % (what, err, tol))
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("d,kind,len_in", [(d, k, 0.0) for d in (8, 24, 200, 257) for k in (0, 1, 2)] + [(520, 1, 0.0), (24, 0, 1.0), (24, 1, 1.0), (24, 2, 1.0)])
def test_fit(eng, d, kind, len_in):
    rng = np.random.default_rng(100 * d + kind)
    x, lab, dout = _fit_data(d, rng)
    n = x.shape[0]
    got = _fit_case(eng, kind, x, lab, dout, len_in)
    ref_m = np.asarray(np.mean(x.astype(np.longdouble), axis=0), np.float64)
    assert np.all(np.abs(got["m_in"] - ref_m) <= 2 * (n + 2) * 2.0 ** -53 * np.mean(np.abs(x), axis=0))
    ref, ref_eig = em.fit(x, lab, kind, d if kind == 0 else dout, len_in, 1.0)
    m_ref, mu, Cm, W, B = em.scatter(x, lab if kind == 2 else None, len_in)
    A = got["A"] if kind else None
    if kind:
        assert A.shape == (dout, d)
        _close(got["eig"], ref_eig, "eigenvalues")
        _close(A.T @ A, ref.A.T @ ref.A, "A^T A")
        _close(A @ (Cm if kind == 1 else W) @ A.T, np.eye(dout), "A S A^T = I")
        if kind == 2:
            _close(A @ B @ A.T, np.diag(ref_eig), "A B A^T = diag(e)")
    else:
        assert got["A"].size == 0
    # m_out = A mu (mu itself for kind 0).  The device's own mu: the column mean of the training rows after steps 1-2 on the device
    chain = eng.embedding
    from plda_amd.embed import EmbeddingChain
    eng.set_embedding(EmbeddingChain(chain.m_in, len_in, None, None, 0.0))
    v_dev = eng.embed(x)
    mu_dev = np.asarray(np.mean(v_dev.astype(np.longdouble), axis=0), np.float64)
    if len_in > 0:
        # mu is a quantity of its own: the issue's band, 1e-8 of the largest element of the reference's A mu
        ref_mo = mu if kind == 0 else ref.A @ mu
        if kind == 0:
            _close(got["m_out"], ref_mo, "m_out = mu")
        else:       # row signs of A are free: through the device's A, and the squared length against the reference's
            assert np.max(np.abs(got["m_out"] - A @ mu)) <= BAND * float(np.max(np.abs(ref_mo)))
            assert abs(got["m_out"] @ got["m_out"] - ref_mo @ ref_mo) <= BAND * float(ref_mo @ ref_mo)
    else:
        # mu is the rounding residue of the centring (1e-16 of the data): no band about it means anything.  What can fail instead:
        # m_out is the sum of the device's own A and the device's own mu, to the rounding of a Din-term fma sum and of the mean (a
        # sequential sum of N terms about the pilot row v_0) ...
        Am = np.eye(d) if kind == 0 else A
        slack = (d + 2) * 2.0 ** -53 * (np.abs(Am) @ np.abs(mu_dev)) + np.abs(Am) @ (2 * (n + 2) * 2.0 ** -53 * (np.mean(np.abs(v_dev), axis=0) + np.abs(v_dev[0])))
        assert np.all(np.abs(got["m_out"] - Am @ mu_dev) <= slack), float(np.max(np.abs(got["m_out"] - Am @ mu_dev) / slack))
        # ... and the training rows, embedded without the last normalisation, have column mean 0 within the band of their size
        eng.set_embedding(EmbeddingChain(chain.m_in, len_in, chain.A, chain.m_out, 0.0))
        u = eng.embed(x)
        assert np.max(np.abs(np.mean(u, axis=0))) <= BAND * float(np.max(np.abs(u)))
    eng.set_embedding(chain)
    if kind and len_in == 0.0:
        shifted = _fit_case(eng, kind, x + 1e5, lab, dout, len_in)
        _close(shifted["A"].T @ shifted["A"], A.T @ A, "A^T A of the data shifted by 1e5")
    if kind == 0:
        return
    # the fitted chain, applied: fp32 rows fitted as fp32 give the chain of their widened copy
    x32 = x.astype(np.float32)
    a = _fit_case(eng, kind, x32, lab, dout, len_in)
    b = _fit_case(eng, kind, x32.astype(np.float64), lab, dout, len_in)
    assert all(_same(a[k], b[k]) for k in a)
    eng.set_embedding(None)


def test_through_liblda(tmp_path):
    from liblda import PLDA
    from conftest import make_data
    rng = np.random.default_rng(21)
    x, y = make_data(3, 600, 40, 40, scale_between=1.0)
    raw = (2.0 * x + 3.0).astype(np.float32)                                    # "extractor output": 40-dimensional, fp32
    y = np.asarray(y).astype(np.uint32)
    p, q = PLDA(), PLDA()
    chain = p.fit_embedding(raw, y, "lda", 24, 1.0, 1.0)
    assert (chain.din, chain.dout) == (40, 24) and p._instance.embedding is chain
    rows = p.embed(raw)
    assert rows.dtype == np.float64 and rows.shape == (600, 24)
    p.fit(raw, y)
    q.fit(rows, y)
    mp, mq = p._instance.get_model(), q._instance.get_model()
    assert all(_same(mp[k], mq[k]) for k in mp)
    tp, tq = p.transform(raw[:300], y[:300]), q.transform(rows[:300], y[:300])
    assert list(tp) == list(tq) and all(tp[k][0] == tq[k][0] and _same(tp[k][1], tq[k][1]) for k in tp)
    ep, eq = p.transform(raw[300:], y[300:]), q.transform(rows[300:], y[300:])
    assert _same(np.asarray(p._instance.score_matrix(tp, ep, znorm=False)), np.asarray(q._instance.score_matrix(tq, eq, znorm=False)))
    offsets = np.array([0, 150, 400, 600], np.int64)
    cp, cq = p.cluster(raw, offsets, 0.0), q.cluster(rows, offsets, 0.0)
    assert _same(cp[0], cq[0]) and _same(cp[1], cq[1])
    dp, dq = p.diarize(raw, offsets, 0.0), q.diarize(rows, offsets, 0.0)
    assert _same(dp[0], dq[0]) and _same(dp[1], dq[1])
    assert _same(p._instance.project_rows(raw), q._instance.project_rows(rows))
    # a chain whose output is not the model's input
    from plda_amd.embed import EmbeddingChain
    p.set_embedding(EmbeddingChain(np.zeros(40), 0.0, np.ones((23, 40)), None, 1.0))
    with pytest.raises(ValueError, match="23.*24"):
        p.cluster(raw, offsets, 0.0)
    p.set_embedding(chain)
    p.save(tmp_path / "with.npz")
    q.save(tmp_path / "without.npz")
    r = PLDA()
    r.load(tmp_path / "with.npz")
    c2 = r._instance.embedding
    assert _same(c2.m_in, chain.m_in) and _same(c2.A, chain.A) and _same(c2.m_out, chain.m_out)
    assert (c2.len_in, c2.len_out) == (chain.len_in, chain.len_out) and _same(r.embed(raw), rows)
    r.load(tmp_path / "without.npz")
    assert r._instance.embedding is None
    with pytest.raises(ValueError):
        r.embed(raw)
    assert r._instance._lib.plda_embed_dims(r._instance._h, None, None, None) == E_NOT_FITTED
