"""GPU: PLDA domain adaptation (csrc/adapt.hip; include/plda_hip.h, "PLDA domain adaptation") against the host model of
tests/adapt_model.py -- the statistics record, its slabs and merges, the shifted-data case, the unsupervised update (Kaldi's
order of operations as the reference), oracle-free invariants, that the new model is the one in use, the blend, every
error of the ABI, poisoned scratch and leaks, and the path through liblda.PLDA.

Shapes: D in {8, 24, 200, 208, 209, 257, 520} (below one 16-tile, C2's size, both sides of the single-workgroup SYRK limit of
208 columns -- the augmented slab is D + 1 wide --, odd D, above the 512 of the block SYRK), N in {1, 15, 17, 1000} around
the SYRK's stage height of 16, and N = 4000 at D = 24."""
import os
import tempfile

import numpy as np
import pytest

import adapt_model as AM
from history_cases import adapt_and_blend_case
from conftest import score_tol

pytestmark = pytest.mark.gpu

DEFAULTS = (0.3, 0.7, 1.0)


def _engine(d, seed, monkeypatch=None, env=None):
    from plda_amd import MPlda
    env = env or {}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = MPlda(0)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    model = AM.synthetic_model(d, seed)
    eng.set_model(*model)
    return eng, model


def _aug(st):
    return AM.augmented(dict(tot_weight=st["tot_weight"], s1=st["s1"], s2=st["s2"]))


def _state(eng):
    """Everything an error must leave bit-identical: the record and the model."""
    st, m = eng.adapt_stats(), eng.get_model()
    return [np.array([st["tot_weight"], st["rows"]]), st["pilot"], st["s1"], st["s2"], m["mean"], m["transform"], m["psi"], m["offset"]]


def _same(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


_gram, _assert_model = AM.gram, AM.assert_model


def _assert_record(st, ref, x, mean, w):
    """the record rule: |delta| <= 1e-12 sum w |x - p|_i |x - p|_j elementwise against the model's record, the pilot the model
    mean, S2 symmetric to the bit"""
    assert st["rows"] == x.shape[0] and np.array_equal(st["pilot"], mean)
    assert (np.abs(_aug(st) - AM.augmented(ref)) <= 1e-12 * AM.record_bound(x, mean, w)).all(), x.shape
    assert np.array_equal(st["s2"], st["s2"].T)


def _domain_rows(model, kind, offset):
    """2 D rows whose second moment about (mean + offset) is EXACTLY C (W + B) C^T in the model's whitened basis: C = 2 I
    ("all": every s = 4 > 1), 0.5 I ("none": every s = 0.25) or alternating 2 / 0.5 ("mixed")."""
    mean, T, psi = model
    d = mean.shape[0]
    W, B = AM.covariances(T, psi)
    L = np.linalg.cholesky(W + B)
    q, _ = np.linalg.qr(np.random.default_rng(d).standard_normal((d, d)))
    c = dict(all=np.full(d, 2.0), none=np.full(d, 0.5), mixed=np.where(np.arange(d) % 2 == 0, 2.0, 0.5))[kind]
    z = np.sqrt(d) * np.concatenate([q, -q]) * c[None, :]
    return mean[None, :] + offset + z @ L.T


# ------------------------------------------------------------------------------------------------------ 1. the record
@pytest.mark.parametrize("d", [8, 24, 200, 208, 209, 257, 520])
def test_record_matches_model(d):
    """|delta| <= 1e-12 sum w |x - p|_i |x - p|_j elementwise (each side's fixed-order fp64 sum is within N 2^-53 <= 4.4e-13 of
    exact for N <= 4000): no weights, random positive weights, some weights exactly zero."""
    eng, (mean, _, _) = _engine(d, 3 * d)
    rng = np.random.default_rng(d)
    for n in (1, 15, 17, 1000) + ((4000,) if d == 24 else ()):
        x = mean[None, :] + 0.7 + rng.standard_normal((n, d))
        wr = rng.random(n) + 0.05
        wz = wr * (rng.random(n) < 0.6)
        for w in (None, wr, wz):
            eng.adapt_reset()
            eng.adapt_accumulate(x, w)
            st = eng.adapt_stats()
            ref = AM.record(x, mean, w)
            _assert_record(st, ref, x, mean, w)


# ------------------------------------------------------------------------------------------------------------ 2. slabs
@pytest.mark.parametrize("d", [24, 209])
def test_slabs_pieces_and_merges(monkeypatch, d):
    import torch
    n = 1000
    rng = np.random.default_rng(50 + d)
    eng, (mean, T, psi) = _engine(d, 9)
    x = mean[None, :] + rng.standard_normal((n, d))
    w = rng.random(n)
    bound = 1e-12 * AM.record_bound(x, mean, w)
    eng.adapt_accumulate(x, w)
    one = eng.adapt_stats()
    # the same call twice: bit-identical
    eng.adapt_reset()
    eng.adapt_accumulate(x, w)
    again = eng.adapt_stats()
    assert _same([_aug(one)], [_aug(again)])
    # the device-pointer form: the same record, bit for bit
    dx, dw = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    torch.cuda.synchronize()
    eng.adapt_reset()
    eng.adapt_accumulate_dev(dx.data_ptr(), n, d, dw.data_ptr())
    assert _same([_aug(one)], [_aug(eng.adapt_stats())])
    # 64 rows per slab against the default
    small, _ = _engine(d, 9, monkeypatch, {"PLDA_ADAPT_SLAB_ROWS": "64"})
    small.adapt_accumulate(x, w)
    assert (np.abs(_aug(small.adapt_stats()) - _aug(one)) <= bound).all()
    # one call in three pieces
    eng.adapt_reset()
    for a, b in ((0, 333), (333, 350), (350, n)):
        eng.adapt_accumulate(x[a:b], w[a:b])
    pieces = eng.adapt_stats()
    assert pieces["rows"] == n and (np.abs(_aug(pieces) - _aug(one)) <= bound).all()
    # two handles merged through get_stats / add_stats
    h1, _ = _engine(d, 9)
    h2, _ = _engine(d, 9)
    h1.adapt_accumulate(x[:600], w[:600])
    h2.adapt_accumulate(x[600:], w[600:])
    s2 = h2.adapt_stats()
    h1.adapt_add_stats(s2["tot_weight"], s2["rows"], s2["pilot"], s2["s1"], s2["s2"])
    merged = h1.adapt_stats()
    assert merged["rows"] == n and (np.abs(_aug(merged) - _aug(one)) <= bound).all()
    # an empty record adopts a pilot that is the model mean
    h3, _ = _engine(d, 9)
    h3.adapt_add_stats(one["tot_weight"], one["rows"], one["pilot"], one["s1"], one["s2"])
    assert _same([_aug(h3.adapt_stats())], [_aug(one)])


def test_scratch_does_not_grow_with_n(monkeypatch):
    """64 rows per slab: the peak of the device bytes over a call at N = 20 000 is no more than the peak at N = 1000 + 64 KiB."""
    from plda_amd import _native
    lib = _native.load()
    d = 24
    rng = np.random.default_rng(1)
    peaks = []
    for n in (1000, 20000):
        eng, (mean, _, _) = _engine(d, 4, monkeypatch, {"PLDA_ADAPT_SLAB_ROWS": "64"})
        x = mean[None, :] + rng.standard_normal((n, d))
        w = rng.random(n)
        eng.synchronize()
        base = lib.plda_device_bytes_held()
        lib.plda_device_bytes_peak(1)
        eng.adapt_accumulate(x, w)
        peaks.append(lib.plda_device_bytes_peak(0) - base)
        del eng
    assert peaks[1] <= peaks[0] + (64 << 10), peaks


# ------------------------------------------------------------------------------------------------------------ 3. shift
def test_shifted_data_keeps_the_variance():
    """Offset 1e5, unit spread, D = 24, N = 4000: the centred variance from the device's record within 1e-10 max|V| of the long
    double one (derived worst case 4.4e-13; Kaldi's sums about 0 lose 7e-5 here, tests/test_adapt_model.py)."""
    from plda_amd import MPlda
    d, n = 24, 4000
    rng = np.random.default_rng(11)
    _, T, psi = AM.synthetic_model(d, 2)
    pilot = 1e5 + rng.random(d)
    x = pilot[None, :] + 0.5 + rng.standard_normal((n, d))
    eng = MPlda(0)
    eng.set_model(pilot, T, psi)
    eng.adapt_accumulate(x)
    st = eng.adapt_stats()
    got = AM.centred_variance(st)
    exact = AM.centred_variance(AM.record(x, pilot, dtype=np.longdouble)).astype(np.float64)
    err = np.abs(got - exact).max()
    print("shift: device %.3g, naive %.3g" % (err, np.abs(AM.naive_variance(x) - exact).max()))
    assert err <= 1e-10 * np.abs(exact).max()


# ------------------------------------------------------------------------------------------------- 4. update vs model
@pytest.mark.parametrize("d", [8, 24, 200, 257, 520])
def test_update_matches_kaldi_order_model(d):
    """In-domain covariance 4 x the model's total (every s > 1), 0.25 x (none), mixed; scales: the defaults, (1, 0, 0),
    (0, 1, 1), (0, 0, 0.5).  mean', T^T T, T^T diag(psi) T, psi and the returned s against Kaldi's order of operations at
    1e-8 max|ref| (the band GetOutput's outputs are held to in tests/test_gpu_fit.py), mean' at 1e-12."""
    eng, model = _engine(d, 17 + d)
    mean, T, psi = model
    offset = 0.05 * np.random.default_rng(d + 1).standard_normal(d)
    for kind, n_excess in (("all", d), ("none", 0), ("mixed", None)):
        x = _domain_rows(model, kind, offset * (0.02 if kind == "none" else 1.0))
        rec = AM.record(x, mean)
        for scales in (DEFAULTS, (1.0, 0.0, 0.0), (0.0, 1.0, 1.0), (0.0, 0.0, 0.5)):
            eng.set_model(mean, T, psi)
            res = eng.adapt(x, None, *scales)
            ref = AM.update_kaldi(mean, T, psi, rec, *scales)
            got = eng.get_model()
            _assert_model(got, ref)
            assert np.abs(res.eigenvalues - ref["s"]).max() <= 1e-8 * np.abs(ref["s"]).max(), (kind, scales)
            if n_excess is not None and scales[2] == 1.0:
                assert res.n_excess == n_excess
            assert res.rows == x.shape[0] and res.tot_weight == float(x.shape[0])
            assert abs(res.mean_shift - np.linalg.norm(ref["mean"] - mean)) <= 1e-10 * max(1.0, res.mean_shift)


# ------------------------------------------------------------------------------------------- 5. oracle-free invariants
@pytest.mark.parametrize("d", [24, 200])
def test_invariants_on_the_device(d):
    eng, model = _engine(d, 71 + d)
    mean, T, psi = model
    x = AM.sample(mean, T, psi, 3 * d + 50, d, scale=1.5, offset=0.3 * np.ones(d))
    tm = T / np.sqrt(1.0 + psi)[:, None]
    # ws + bs = 1: the total covariance gains exactly the excess
    res = eng.adapt(x)
    m = eng.get_model()
    Wn, Bn = AM.covariances(m["transform"], m["psi"])
    lam = np.sort(np.linalg.eigvalsh(tm @ (Wn + Bn) @ tm.T))[::-1]
    want = np.maximum(res.eigenvalues, 1.0)
    assert 0 < res.n_excess and np.abs(lam - want).max() <= 1e-8 * want.max()
    # again on the same rows: the data no longer exceeds the model
    res2 = eng.adapt(x)
    m2 = eng.get_model()
    assert np.abs(m2["psi"] - m["psi"]).max() <= 1e-8 * np.abs(m["psi"]).max()
    assert (res2.eigenvalues - 1.0).max() <= 1e-8
    # ws = bs = 0: only the mean moves
    eng.set_model(mean, T, psi)
    eng.adapt(x, None, 0.0, 0.0, 1.0)
    m0 = eng.get_model()
    g1, g2 = _gram(m0["transform"], m0["psi"])
    r1, r2 = _gram(T, psi)
    assert np.abs(g1 - r1).max() <= 1e-8 * np.abs(r1).max() and np.abs(g2 - r2).max() <= 1e-8 * np.abs(r2).max()
    assert np.abs(m0["psi"] - psi).max() <= 1e-8 * psi.max()
    assert np.abs(m0["mean"] - x.mean(0)).max() <= 1e-12 * np.abs(x.mean(0)).max()


# ------------------------------------------------------------------------------------ 6. the new model is the one in use
def test_new_model_is_the_one_in_use():
    import torch
    from oracle import plda_oracle_np as onp
    from plda_amd.calibration import Calibration
    d, m, nt = 24, 40, 40
    eng, model = _engine(d, 5)
    mean, T, psi = model
    rng = np.random.default_rng(8)
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    counts = np.where(np.arange(m) % 2 == 0, 2, 5).astype(np.int32)
    # state that describes the old model: z-norm maps, a calibration, a prepared test side
    eng._meanz, eng._stdvz = {1: 0.5}, {1: 2.0}
    eng._calibration = Calibration(1.0, 0.0, 0.5)
    dU, dV = torch.from_numpy(U).cuda(), torch.from_numpy(V).cuda()
    old = torch.empty((m, nt), dtype=torch.float32, device="cuda")
    new = torch.empty_like(old)
    torch.cuda.synchronize()
    eng.score_prepare_dev(dV.data_ptr(), nt, mixed_counts=False, n_uniform=3)
    eng.score_matrix_dev(dU.data_ptr(), None, 3, m, dV.data_ptr(), nt, old.data_ptr(), nt)
    eng.synchronize()
    x = AM.sample(mean, T, psi, 200, 3, scale=2.0, offset=0.2 * np.ones(d))
    eng.adapt(x)
    g = eng.get_model()
    assert np.abs(g["psi"] - psi).max() > 1e-3
    off = -g["transform"] @ g["mean"]
    assert np.abs(g["offset"] - off).max() <= 1e-12 * (np.abs(g["transform"]) @ np.abs(g["mean"])).max()
    assert eng._meanz == {} and eng._stdvz == {} and eng._calibration is None and eng._zn_tag is None
    # the prepared side is not reused: the same pointers now give the scores of the NEW model (the old ones are not them)
    eng.score_matrix_dev(dU.data_ptr(), None, 3, m, dV.data_ptr(), nt, new.data_ptr(), nt)
    eng.synchronize()
    ref3 = onp.llr_matrix(g["psi"], U, 3, V)
    assert (np.abs(new.cpu().numpy() - ref3) <= score_tol(ref3)).all()
    assert not (np.abs(old.cpu().numpy() - ref3) <= score_tol(ref3)).all()
    # score_matrix with two distinct enrol counts and score() against the oracle on get_model()
    S = eng.score_matrix((counts, U), (np.ones(nt, np.int32), V))
    ref = onp.llr_matrix(g["psi"], U, counts, V)
    assert (np.abs(S - ref) <= score_tol(ref)).all()
    one = np.array([[eng.score(7, (int(counts[i]), U[i]), (1, V[j])) for j in range(3)] for i in range(4)])
    assert (np.abs(one - ref[:4, :3]) <= score_tol(ref)[:4, :3]).all()


# ------------------------------------------------------------------------------------------------------------ 7. blend
@pytest.mark.parametrize("d", [24, 257])
def test_blend(d):
    eng, a = _engine(d, 1)
    b = AM.synthetic_model(d, 2)
    eng.blend(b, 0.0)
    _assert_model(eng.get_model(), dict(mean=a[0], transform=a[1], psi=a[2]))
    eng.set_model(*a)
    eng.blend(b, 1.0)
    _assert_model(eng.get_model(), dict(mean=b[0], transform=b[1], psi=b[2]))
    eng.set_model(*a)
    eng.blend(b, 0.5)
    _assert_model(eng.get_model(), AM.blend(a, b, 0.5))
    # alpha_mean is independent of alpha; the other model as an MPlda
    from plda_amd import MPlda
    other = MPlda(0)
    other.set_model(*b)
    eng.set_model(*a)
    eng._meanz, eng._stdvz = {3: 1.0}, {3: 1.0}
    eng.blend(other, 0.25, 1.0)
    _assert_model(eng.get_model(), AM.blend(a, b, 0.25, 1.0))
    assert np.abs(eng.get_model()["mean"] - b[0]).max() <= 1e-15 and eng._meanz == {}
    g = eng.get_model()
    assert np.abs(g["offset"] + g["transform"] @ g["mean"]).max() <= 1e-12 * (np.abs(g["transform"]) @ np.abs(g["mean"])).max()


# ----------------------------------------------------------------------------------------------------------- 8. errors
def test_errors_leave_record_and_model_untouched():
    from plda_amd import MPlda
    from plda_amd._native import PldaError, PLDA_E_INVAL, PLDA_E_NOT_FITTED
    d = 24
    rng = np.random.default_rng(2)
    empty = MPlda(0)
    with pytest.raises(PldaError) as e:
        empty.adapt_accumulate(np.zeros((3, d)))
    assert e.value.code == PLDA_E_NOT_FITTED
    eng, (mean, T, psi) = _engine(d, 6)
    x = mean[None, :] + rng.standard_normal((100, d))
    w = rng.random(100)

    def refused(call, match, code=PLDA_E_INVAL):
        before = _state(eng)
        with pytest.raises(PldaError, match=match) as err:
            call()
        assert err.value.code == code
        assert _same(before, _state(eng)), match

    for seeded in (False, True):          # on an empty record, then on one that holds rows
        eng.adapt_reset()
        if seeded:
            eng.adapt_accumulate(x, w)
        bad = x.copy(); bad[7, 3] = np.nan; bad[50, 0] = np.inf
        refused(lambda: eng.adapt_accumulate(bad, w), "2 row")
        wn = w.copy(); wn[4] = -1e-3; wn[5] = np.nan; wn[6] = np.inf
        refused(lambda: eng.adapt_accumulate(x, wn), "3 negative or non-finite weight")
        refused(lambda: eng.adapt_accumulate(np.zeros((5, d + 1))), "feature dim")
        refused(lambda: eng._ck(eng._lib.plda_adapt_accumulate(eng._h, x.ctypes.data, -1, d, None)), "N = -1")
        refused(lambda: eng.adapt_update(-0.1, 0.7, 1.0), "scales")
        other_pilot = mean.copy(); other_pilot[0] = np.nextafter(other_pilot[0], 2.0)
        refused(lambda: eng.adapt_add_stats(1.0, 1, other_pilot, np.zeros(d), np.zeros((d, d))), "pilot differs")
        if not seeded:
            refused(lambda: eng.adapt_update(), "no statistics")
            eng.adapt_accumulate(np.zeros((0, d)))          # N == 0: nothing happens
            eng.adapt_accumulate(x, np.zeros(100))          # total weight 0
            refused(lambda: eng.adapt_update(), "no statistics")
    # the model changed since the pilot
    eng.set_model(mean + 1.0, T, psi)
    refused(lambda: eng.adapt_accumulate(x), "reset first")
    refused(lambda: eng.adapt_update(), "reset first")
    # a second update on the same record
    eng.adapt_reset()
    eng.adapt_accumulate(x + 1.0)
    eng.adapt_update()
    refused(lambda: eng.adapt_update(), "reset first")
    refused(lambda: eng.adapt_accumulate(x), "reset first")
    # blend: dimension, range, a singular second model
    b = AM.synthetic_model(d, 9)
    refused(lambda: eng.blend(AM.synthetic_model(d + 1, 9), 0.5), "dimension")
    refused(lambda: eng.blend(b, 1.5), "alpha")
    refused(lambda: eng.blend(b, 0.5, -0.1), "alpha")
    from plda_amd._native import PLDA_E_NUMERIC
    refused(lambda: eng.blend((b[0], np.zeros((d, d)), b[2]), 0.5), "blend_model", PLDA_E_NUMERIC)
    # a truncated model has no covariances
    eng.truncate(d - 4)
    with pytest.raises(PldaError, match="adapt before truncating"):
        eng.adapt_accumulate(x)
    with pytest.raises(PldaError, match="adapt before truncating"):
        eng.adapt_update()
    with pytest.raises(PldaError, match="adapt before truncating"):
        eng.blend(b, 0.5)


def test_stats_of_a_record_of_another_dimension_are_refused():
    """get_stats writes D and D x D doubles with D the MODEL's dimension, the only one the caller can size its arrays from:
    once the model is replaced by one of another dimension the old record must be refused, not copied out at its own size."""
    from plda_amd._native import PldaError, PLDA_E_INVAL
    eng, (mean, T, psi) = _engine(24, 11)
    eng.adapt_accumulate(mean[None, :] + np.random.default_rng(0).standard_normal((50, 24)))
    eng.set_model(mean + 1.0, T, psi)                 # same dimension: stale, but still readable
    assert eng.adapt_stats()["rows"] == 50
    small = AM.synthetic_model(8, 12)
    eng.set_model(*small)
    with pytest.raises(PldaError, match="reset first") as err:
        eng.adapt_stats()
    assert err.value.code == PLDA_E_INVAL
    with pytest.raises(PldaError, match="reset first"):
        eng.adapt_accumulate(small[0][None, :])
    eng.adapt_reset()
    st = eng.adapt_stats()
    assert st["rows"] == 0 and st["s2"].shape == (8, 8) and np.array_equal(st["pilot"], small[0])


def test_update_and_blend_state_their_size_limit():
    """D > 2048 is past both eigensolvers: refused up front with adapt's own message, the model untouched."""
    from plda_amd import MPlda
    from plda_amd._native import PldaError, PLDA_E_INVAL
    d = 2049
    model = (np.linspace(-1.0, 1.0, d), np.diag(np.linspace(0.5, 1.5, d)), np.linspace(3.0, 0.05, d))
    eng = MPlda(0)
    eng.set_model(*model)
    for call in (lambda: eng.adapt_update(), lambda: eng.blend(model, 0.5)):
        with pytest.raises(PldaError, match="supported up to D = 2048") as err:
            call()
        assert err.value.code == PLDA_E_INVAL
    m = eng.get_model()
    assert np.array_equal(m["transform"], model[1]) and np.array_equal(m["psi"], model[2])


# ------------------------------------------------------------------------------------------ 9. poisoned scratch, leaks
def _twice(monkeypatch, case):
    from plda_amd import MPlda
    out = {}
    for poison in (False, True):
        if poison:
            monkeypatch.setenv("PLDA_SCRATCH_POISON", "1")
        else:
            monkeypatch.delenv("PLDA_SCRATCH_POISON", raising=False)
        eng = MPlda(0)
        monkeypatch.delenv("PLDA_SCRATCH_POISON", raising=False)
        out[poison] = {k: np.asarray(v).copy() for k, v in case(eng).items()}
        eng.synchronize()
        del eng
    MPlda(0)                       # the switch off again for whatever runs next in this process
    for k, a in out[False].items():
        b = out[True][k]
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), \
            "%s differs on poisoned scratch (NaN on poisoned: %d)" % (k, int(np.isnan(b).sum()))
    return out[False]


@pytest.mark.parametrize("d", [24, 257])
def test_adapt_and_blend_on_poisoned_scratch(monkeypatch, d):
    model = AM.synthetic_model(d, 40 + d)
    other = AM.synthetic_model(d, 41 + d)
    x = AM.sample(*model, 333, d, scale=1.4, offset=0.1 * np.ones(d))
    w = np.random.default_rng(d).random(333)

    case = adapt_and_blend_case(model, other, x, w)        # (shared with tests/test_gpu_handle_history.py)
    a = _twice(monkeypatch, case)
    ref = AM.update_kaldi(*model, AM.record(x, model[0], w))
    _assert_model(dict(mean=a["mean"], transform=a["T"], psi=a["psi"]), ref)
    _assert_model(dict(mean=a["bmean"], transform=a["bT"], psi=a["bpsi"]),
                  AM.blend((ref["mean"], ref["transform"], ref["psi"]), other, 0.3, 0.6))


def test_create_adapt_destroy_gives_every_byte_back():
    from plda_amd import MPlda, _native
    lib = _native.load()
    d = 24
    model, other = AM.synthetic_model(d, 1), AM.synthetic_model(d, 2)
    x = AM.sample(*model, 200, 1, scale=1.5)
    start = lib.plda_device_bytes_held()
    for _ in range(10):
        eng = MPlda(0)
        eng.set_model(*model)
        eng.adapt(x)
        eng.blend(other, 0.5)
        eng.synchronize()
        del eng
    assert lib.plda_device_bytes_held() == start


# ------------------------------------------------------------------------------------------------------- 10. end to end
def test_end_to_end_through_liblda():
    from liblda import PLDA
    from conftest import make_data
    d = 24
    x, y = make_data(5, 300, d, 60, scale_between=0.5)
    rng = np.random.default_rng(6)
    z = 0.4 + 3.0 * rng.random((500, d))
    p = PLDA()
    p.fit(x, y, 5)
    before = p._instance.get_model()
    res = p.adapt(z)
    st = p._instance.adapt_stats()
    assert res.rows == st["rows"] == 500 and res.tot_weight == st["tot_weight"] == 500.0
    assert res.eigenvalues.shape == (d,) and (np.diff(res.eigenvalues) <= 0).all()
    assert res.n_excess == int((res.eigenvalues > 1.0).sum()) and res.n_excess > 0
    assert abs(res.mean_shift - np.linalg.norm(st["s1"] / st["tot_weight"])) <= 1e-12 * res.mean_shift
    after = p._instance.get_model()
    assert np.abs(after["mean"] - z.mean(0)).max() <= 1e-12
    ref = AM.update_kaldi(before["mean"], before["transform"], before["psi"], AM.record(z, before["mean"]))
    _assert_model(after, ref)
    labels = (np.arange(500) % 50).astype(np.uint64)
    enrol, test = p.transform(z[:250], labels[:250]), p.transform(z[250:], labels[250:])
    S = p.score_matrix(enrol, test)
    assert np.isfinite(S).all()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "adapted.plda")
        p.save_kaldi(path)
        q = PLDA().load_kaldi(path)
    S2 = q.score_matrix(q.transform(z[:250], labels[:250]), q.transform(z[250:], labels[250:]))
    assert np.array_equal(S, S2)
    # blend through the public class: half way back to the out-of-domain model
    p.blend((before["mean"], before["transform"], before["psi"]), 0.5)
    _assert_model(p._instance.get_model(),
                  AM.blend((after["mean"], after["transform"], after["psi"]), (before["mean"], before["transform"], before["psi"]), 0.5))
