"""GPU: the ROC convex hull (csrc/rocch.hip) against the sort-based host model tests/rocch_model.py.  Vertices (counts, key,
threshold), the reduced points and every count are compared with ==; min_cllr within 1e-12 absolute (the band the calibration
derived for fp64 sums of a few hundred log1p terms at an ulp each); the ROCCH-EER within 4 ulp of the exact rational; the three
PLDA_ROCCH_VARIANT arms bit-identical.  Then the relations to the merged code (calibration pass, minDCF, affine fit), the PAV
map, refusals, guard bands, poisoned scratch, a long-lived handle, and PLDA.min_cllr / calibrate_pav on a fitted model."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import rocch_model as RM

pytestmark = pytest.mark.gpu

ENV = ("PLDA_EER_SLAB_ROWS", "PLDA_SCRATCH_POISON", "PLDA_ROCCH_VARIANT", "PLDA_ROCCH_EDGE_CAP", "PLDA_MINDCF_VARIANT", "PLDA_EER_VARIANT")
GUARD_BYTES = 64 << 10


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _make(variant=0, d=0, slab=None, poison=False, cap=None):
    """a fresh handle made with the suite's creation-time switches cleared around it, but these"""
    from plda_amd import MPlda
    saved = {k: os.environ.pop(k, None) for k in ENV}
    try:
        if variant:
            os.environ["PLDA_ROCCH_VARIANT"] = str(variant)
        if slab:
            os.environ["PLDA_EER_SLAB_ROWS"] = str(slab)
        if poison:
            os.environ["PLDA_SCRATCH_POISON"] = "1"
        if cap:
            os.environ["PLDA_ROCCH_EDGE_CAP"] = str(cap)
        eng = MPlda(0)
    finally:
        for k in ENV:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    if d:
        rng = np.random.default_rng(d)
        q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        eng.set_model(rng.random(d), q * (1.0 + rng.random(d))[:, None], np.sort(0.05 + rng.random(d) * 4.0)[::-1].copy())
    return eng


@pytest.fixture(scope="module")
def engines():
    """one handle per PLDA_ROCCH_VARIANT arm: unset, 1 (no LDS window), 2 (a window of 256 gaps)"""
    return {v: _make(v) for v in (0, 1, 2)}


def _split(S, es, ts):
    tgt = np.asarray(es)[:, None] == np.asarray(ts)[None, :]
    return S[tgt], S[~tgt]


def _flat(res, pav, info):
    """everything a call returns, as arrays (bit-wise comparisons between arms, runs and handles)"""
    out = {"f": np.array([res[k] for k in ("min_cllr", "eer", "eer_far_lo", "eer_far_hi", "eer_frr_lo", "eer_frr_hi")], np.float64),
           "c": np.array([res["Np"], res["Nn"], res["n_vertices"], info["t_raw"], info["t_distinct"], info["edge_class"]], np.int64),
           "v": pav.vertices.copy(), "l": pav.llr.copy()}
    if "points" in info:
        for k in ("edge_key", "other_lt", "other_le", "edge_lt", "edge_le"):
            out["p_" + k] = info["points"][k]
    return out


def _same_bits(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), (what, k)


def _check(got, pos, neg, what, model=None):
    """one call's (result, pav, info) == the model of (pos, neg)"""
    res, pav, info = got
    m = model or RM.model(pos, neg)
    print("%s: Np %d Nn %d vertices %d min_cllr %.17g (model %.17g) eer %.17g (model %.17g) T %d window %d+%d lds %d atomics %d registers %d reads %d" % (
        what, res["Np"], res["Nn"], res["n_vertices"], res["min_cllr"], m["min_cllr"], res["eer"], float(m["eer"]), info["t_distinct"],
        info["window_start"], info["window_size"], info["n_lds"], info["n_global_atomic"], info["n_register"], info["reads"]))
    assert (res["Np"], res["Nn"], res["n_vertices"]) == (len(pos), len(neg), len(m["vertices"]))
    v = pav.vertices
    got_v = [(int(r["x"]), int(r["y"]), int(r["fa"]), int(r["miss"]), int(r["key"]), int(r["has_key"]), float(r["threshold"])) for r in v]
    assert got_v == m["vertices"], what
    assert len(pav.llr) == len(m["llr"])
    for a, b in zip(pav.llr, m["llr"]):
        assert a == b if math.isinf(b) else abs(a - b) <= 1e-12 * max(1.0, abs(b))
    assert abs(res["min_cllr"] - m["min_cllr"]) <= 1e-12
    assert RM.ulp_distance(res["eer"], float(m["eer"])) <= 4
    Np, Nn = len(pos), len(neg)
    assert (res["eer_far_lo"], res["eer_frr_lo"]) == ((Nn - m["eer_lo"][0]) / Nn, m["eer_lo"][1] / Np)
    assert (res["eer_far_hi"], res["eer_frr_hi"]) == ((Nn - m["eer_hi"][0]) / Nn, m["eer_hi"][1] / Np)
    if "points" in info:
        ec, u, olt, ole, elt, ele = RM.reduced_points(pos, neg)
        p = info["points"]
        assert (p["edge_class"], p["T"], info["edge_class"], info["t_distinct"], info["t_raw"]) == (ec, len(u), ec, len(u), min(Np, Nn))
        for name, ref in (("edge_key", u), ("other_lt", olt), ("other_le", ole), ("edge_lt", elt), ("edge_le", ele)):
            assert np.array_equal(p[name], ref), (what, name)
    other = max(Np, Nn)
    assert info["n_lds"] + info["n_global_atomic"] + info["n_register"] == other
    return m


def _matrix(eng, S, nt, es, ts, off=0, points=True):
    """S [m, ld] holds the matrix in its first nt columns; off: the matrix starts that many floats into its buffer"""
    import torch
    from plda_amd import rocch as R
    dS, des, dts = _t(np.concatenate([np.zeros(off, np.float32), S.ravel()])), _t(np.asarray(es, np.int64)), _t(np.asarray(ts, np.int64))
    torch.cuda.synchronize()
    return R.rocch_from_matrix_dev(eng, dS.data_ptr() + 4 * off, S.shape[1], S.shape[0], nt, des.data_ptr(), dts.data_ptr(), points=points)


def _all_arms(engines, call, pos, neg, what):
    """the call under the three arms: each equals the model, and they agree bit for bit"""
    m, first = None, None
    for v, eng in engines.items():
        got = call(eng)
        m = _check(got, pos, neg, "%s, variant %d" % (what, v), m)
        flat = _flat(*got)
        if first is None:
            first = flat
        else:
            _same_bits(flat, first, "%s: variant %d against the default" % (what, v))
    return got


def _lists_all_arms(engines, pos, neg, what):
    from plda_amd import rocch as R
    pos, neg = np.asarray(pos, np.float32), np.asarray(neg, np.float32)
    return _all_arms(engines, lambda eng: R.rocch_from_lists(eng, pos, neg, points=True), pos, neg, what)


# ---------------------------------------------------------------------------------------------- matrix edges
@pytest.mark.parametrize("nt", [1, 3, 1023, 1024, 1025, 2049])
def test_matrix_edges(engines, nt):
    """M in {1, 5, 17}; the scalar path (a pitch that is no multiple of 4, a base off the 16-byte boundary) and its aligned twin"""
    from plda_amd._native import PldaError
    for m in (1, 5, 17):
        rng = np.random.default_rng(1000 * nt + m)
        es, ts = rng.integers(0, 3, m), rng.integers(0, 3, nt)
        es[0] = ts[0] = 0
        if nt > 1:
            ts[-1] = 99
        elif m > 1:
            es[1:] = 7
        quant = (0.0, 0.25, 1.0)[(nt + m) % 3]
        for ld, off in ((nt + 4 - nt % 4 + 1, 1), ((nt + 3) // 4 * 4, 0)):
            S = rng.standard_normal((m, ld)).astype(np.float32)
            S[:, :nt] += np.float32(1.5) * (es[:, None] == ts[None, :])
            if quant:
                S = (np.round(S / quant) * quant).astype(np.float32)
            if m * nt == 1:
                with pytest.raises(PldaError, match="at least one target") as e:
                    _matrix(engines[0], S, nt, es, ts, off)
                assert e.value.code == -1
                continue
            pos, neg = _split(S[:, :nt], es, ts)
            _all_arms(engines, lambda eng: _matrix(eng, S, nt, es, ts, off), pos, neg, "%d x %d, ld %d, offset %d" % (m, nt, ld, off))


# ---------------------------------------------------------------------------------------------- ties, closed forms, extreme scores
def test_ties_and_closed_forms(engines):
    rng = np.random.default_rng(2)
    for quant in (0.25, 1.0):
        pos = np.round(rng.normal(1.0, 1.0, 700) / quant) * quant
        neg = np.round(rng.normal(0.0, 1.0, 5000) / quant) * quant
        _lists_all_arms(engines, pos, neg, "scores rounded to %g" % quant)
    res, pav, _ = _lists_all_arms(engines, [0.5] * 40, [0.5] * 300, "every score equal")
    assert res["n_vertices"] == 2 and res["min_cllr"] == 1.0 and list(pav.llr) == [0.0]
    res, pav, _ = _lists_all_arms(engines, rng.uniform(5, 6, 50), rng.uniform(-1, 1, 900), "separated")
    assert res["n_vertices"] == 3 and res["min_cllr"] == 0.0 and list(pav.llr) == [-math.inf, math.inf] and res["eer"] == 0.0
    res, _, _ = _lists_all_arms(engines, rng.uniform(-6, -5, 50), rng.uniform(-1, 1, 900), "targets all below")
    assert res["n_vertices"] == 2 and res["min_cllr"] == 1.0 and res["eer"] == 0.5
    fmax, den = np.finfo(np.float32).max, np.float32(1e-45)
    pos = np.float32([0.0, -0.0, den, fmax, 1.0, -den, 2 * den])
    neg = np.float32([-0.0, 0.0, -den, -fmax, den, 1.0, fmax, -fmax, 0.0, 3 * den])
    _lists_all_arms(engines, pos, neg, "+-0, denormals, +-FLT_MAX")
    S = np.concatenate([pos, neg])[None, :]
    ts = np.concatenate([np.zeros(len(pos), np.int64), np.ones(len(neg), np.int64)])
    _all_arms(engines, lambda eng: _matrix(eng, S, S.shape[1], [0], ts), pos, neg, "the same as a matrix")


# ---------------------------------------------------------------------------------------------- the edge class
@pytest.mark.parametrize("npos,nneg", [(300, 4000), (4000, 300), (1500, 1500), (1, 30000), (30000, 1)])
def test_edge_class_of_lists(engines, npos, nneg):
    rng = np.random.default_rng(npos + nneg)
    got = _lists_all_arms(engines, rng.normal(1.0, 1.0, npos), rng.normal(0.0, 1.0, nneg), "%d against %d" % (npos, nneg))
    assert got[2]["edge_class"] == (1 if npos <= nneg else 0)


def test_edge_class_of_matrices(engines):
    rng = np.random.default_rng(8)
    m, nt = 60, 1100                                     # two speakers: half the trials are targets
    for flip in (0, 1):                                  # ... a few more / a few less than half: both edge classes
        es, ts = rng.integers(0, 2, m), rng.integers(0, 2, nt)
        es[:40], ts[:700] = 0, flip
        S = (rng.standard_normal((m, nt)) + 1.0 * (es[:, None] == ts[None, :])).astype(np.float32)
        pos, neg = _split(S, es, ts)
        got = _all_arms(engines, lambda eng: _matrix(eng, S, nt, es, ts), pos, neg, "two speakers, Np %d Nn %d" % (len(pos), len(neg)))
        assert got[2]["edge_class"] == (1 if len(pos) <= len(neg) else 0)
    es, ts = np.arange(m) + 1000, np.arange(nt) + 5000  # all distinct, one match
    es[17] = ts[1030] = 3
    S = rng.standard_normal((m, nt)).astype(np.float32)
    pos, neg = _split(S, es, ts)
    got = _all_arms(engines, lambda eng: _matrix(eng, S, nt, es, ts), pos, neg, "one target")
    assert got[0]["Np"] == 1 and got[2]["t_raw"] == 1


# ---------------------------------------------------------------------------------------------- the window
@pytest.mark.parametrize("T", [255, 256, 257, 1000])
def test_window_of_256_gaps(engines, T):
    """the other class's mass below, inside, astride and above the window (variant 2: 256 gaps)"""
    rng = np.random.default_rng(T)
    pos = np.sort(rng.normal(0.0, 1.0, T)).astype(np.float32)
    for where, centre, width in (("low", 0.05, 0.02), ("middle", 0.5, 0.02), ("astride", 0.5, 0.6), ("high", 0.95, 0.02)):
        q = np.clip(rng.normal(centre, width, 6000), 0.0, 1.0)
        cluster = np.quantile(pos.astype(np.float64), q)
        back = rng.uniform(pos[0] - 0.5, pos[-1] + 0.5, 3000)
        neg = np.concatenate([cluster + rng.normal(0.0, 1e-3, 6000), back]).astype(np.float32)
        got = _lists_all_arms(engines, pos, neg, "T %d, mass %s" % (T, where))
        from plda_amd import rocch as R
        _, _, i2 = R.rocch_from_lists(engines[2], pos, neg)
        _, _, i1 = R.rocch_from_lists(engines[1], pos, neg)
        assert i1["n_lds"] == 0 and i1["window_size"] == 0 and i1["coarse_read"] == 0
        assert i2["window_size"] == 256
        if T > 256:
            assert i2["coarse_read"] == 1 and i2["n_lds"] > 0 and 0 <= i2["window_start"] <= T - 256
            # (T = 257 leaves one gap outside the window, which may hold nothing; T = 1000 leaves 744 under a uniform background)
            assert i2["n_global_atomic"] > 0 or T == 257
            if where != "astride":
                assert i2["n_lds"] > i2["n_global_atomic"]       # the window found the cluster
        else:
            assert i2["coarse_read"] == 0 and i2["n_global_atomic"] == 0
        del got


def test_real_window_300_x_300_two_speakers(engines):
    rng = np.random.default_rng(300)
    es, ts = rng.integers(0, 2, 300), rng.integers(0, 2, 300)
    S = (rng.standard_normal((300, 300)) + 1.0 * (es[:, None] == ts[None, :])).astype(np.float32)
    pos, neg = _split(S, es, ts)
    got = _all_arms(engines, lambda eng: _matrix(eng, S, 300, es, ts), pos, neg, "300 x 300")
    info = _matrix(engines[0], S, 300, es, ts, points=False)[2]
    assert info["t_raw"] > 4096 and info["window_size"] == 4096 and info["coarse_read"] == 1
    assert info["n_lds"] > 0 and info["n_global_atomic"] > 0
    del got


def test_duplicated_edge_keys(engines):
    rng = np.random.default_rng(4)
    pos = np.repeat(rng.normal(1.0, 1.0, 90).astype(np.float32), rng.integers(1, 9, 90))
    neg = np.concatenate([rng.normal(0.0, 1.0, 3000).astype(np.float32), pos[::3]])
    got = _lists_all_arms(engines, pos, neg, "multiplicities above 1")
    assert got[2]["t_distinct"] == 90 < got[2]["t_raw"]
    got = _lists_all_arms(engines, [0.25] * 500, np.concatenate([rng.normal(0.0, 1.0, 3000), [0.25] * 7]), "all T equal")
    assert got[2]["t_distinct"] == 1 and got[2]["t_raw"] == 500


# ---------------------------------------------------------------------------------------------- the operand form
@pytest.mark.parametrize("mixed,zn,m,nt", [(False, False, 900, 1300), (True, True, 900, 1300), (True, True, 513, 1025)],
                         ids=["False-False", "True-True", "True-True-513x1025"])
def test_operand_form_is_score_matrix_plus_matrix_form(mixed, zn, m, nt):
    import torch
    from plda_amd import rocch as R
    d = 48
    eng = _make(d=d, slab=256)                  # 900 rows: four slabs; 513 rows: three, the last of one row
    rng = np.random.default_rng(41 + mixed)
    spk = rng.standard_normal((30, d)) * 1.5
    es, ts = rng.integers(0, 30, m), rng.integers(0, 30, nt)
    U, V = spk[es] + rng.standard_normal((m, d)), spk[ts] + rng.standard_normal((nt, d))
    n = rng.integers(1, 4, m).astype(np.int32)
    dU, dV, des, dts = _t(U), _t(V), _t(es.astype(np.int64)), _t(ts.astype(np.int64))
    dn = _t(n) if mixed else None
    nu = 0 if mixed else 2
    dzm, dzs = (_t(rng.standard_normal(m)), _t(0.5 + rng.random(m))) if zn else (None, None)
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    S = torch.empty((m, nt), dtype=torch.float32, device=_dev())
    torch.cuda.synchronize()
    eng.score_matrix_dev(dU.data_ptr(), ptr(dn), nu, m, dV.data_ptr(), nt, S.data_ptr(), nt, ptr(dzm), ptr(dzs))
    eng.synchronize()
    mat = R.rocch_from_matrix_dev(eng, S.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr(), points=True)
    opr = R.rocch_from_operands_dev(eng, dU.data_ptr(), ptr(dn), nu, m, dV.data_ptr(), nt, des.data_ptr(), dts.data_ptr(), ptr(dzm), ptr(dzs),
                                    points=True)
    opr2 = R.rocch_from_operands_dev(eng, dU.data_ptr(), ptr(dn), nu, m, dV.data_ptr(), nt, des.data_ptr(), dts.data_ptr(), ptr(dzm), ptr(dzs),
                                     points=True)
    _same_bits(_flat(*opr), _flat(*mat), "operand form against matrix form")
    _same_bits(_flat(*opr2), _flat(*opr), "operand form again")
    if m == 513:
        pos, neg = _split(S.cpu().numpy(), es, ts)
        _check(mat, pos, neg, "matrix form")
    print(opr[2])


# ---------------------------------------------------------------------------------------------- cross-checks against merged code
def test_cross_checks_against_calibration_and_min_dcf(engines):
    from plda_amd import calibration as CB
    from plda_amd import dcf as DC
    eng = engines[0]
    rng = np.random.default_rng(77)
    m, nt, k = 400, 700, 12
    es, ts = rng.integers(0, k, m), rng.integers(0, k, nt)
    S = (rng.standard_normal((m, nt)) * 3.0 + 6.0 * (es[:, None] == ts[None, :])).astype(np.float32)
    dS, des, dts = _t(S), _t(es.astype(np.int64)), _t(ts.astype(np.int64))
    args = (dS.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr())
    from plda_amd import rocch as R
    res, pav, _ = R.rocch_from_matrix_dev(eng, *args)
    pos, neg = _split(S, es, ts)
    _check((res, pav, {"t_distinct": 0, "window_start": 0, "window_size": 0, "n_lds": len(neg), "n_global_atomic": 0, "n_register": 0, "reads": 0}),
           pos, neg, "400 x 700")
    Np, Nn = res["Np"], res["Nn"]
    # every vertex's (miss, fa) is what a calibration pass counts at its threshold
    for v in pav.vertices:
        rec = CB.pass_from_matrix_dev(eng, *args, theta=float(v["threshold"]))
        assert (rec["miss"], rec["fa"]) == (int(v["miss"]), int(v["fa"])), v
    # minDCF <= the best vertex (exact: vertices are cuts) <= minDCF (1 + 2^-49) (the optimum of a linear cost is a vertex)
    pts = ((0.01, 1.0, 1.0), (0.05, 1.0, 1.0), (0.5, 1.0, 1.0), (0.001, 1.0, 1.0), (0.01, 10.0, 1.0))
    got, _ = DC.min_dcf_from_matrix_dev(eng, *args, points=pts)
    for (prior, cm, cf), g in zip(pts, got):
        a, b = cm * prior, cf * (1.0 - prior)
        best = min(min((a * float(int(v["miss"]))) / float(Np) + (b * float(int(v["fa"]))) / float(Nn) for v in pav.vertices) / min(a, b), 1.0)
        print("point %r: min_dcf %.17g best vertex %.17g" % ((prior, cm, cf), g["min_dcf"], best))
        assert g["min_dcf"] <= best <= g["min_dcf"] * (1.0 + 2.0 ** -49)
    # the floor under the affine calibration
    fit = CB.fit_from_matrix_dev(eng, *args)
    cllr_after = fit["cllr_after"] if isinstance(fit, dict) else fit.cllr_after
    print("min_cllr %.17g cllr_after %.17g" % (res["min_cllr"], cllr_after))
    assert res["min_cllr"] <= cllr_after + 1e-12
    # Cllr of the PAV-mapped scores (fp32 map; its infinite end segments clamped to +-60: a cost below 1e-26 per trial)
    import torch
    out = torch.empty_like(dS)
    pav.apply_dev(eng, dS.data_ptr(), nt, m, nt, out.data_ptr(), nt, bound=60.0)
    eng.synchronize()
    mapped = CB.cllr(CB.pass_from_matrix_dev(eng, out.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr()))
    print("Cllr of the mapped scores %.17g" % mapped)
    assert abs(mapped - res["min_cllr"]) <= 1e-6


# ---------------------------------------------------------------------------------------------- the PAV map
def test_pav_map_equals_the_host_map(engines):
    import torch
    from plda_amd import rocch as R
    eng = engines[0]
    rng = np.random.default_rng(6)
    pos, neg = rng.normal(1.0, 1.0, 400).astype(np.float32), rng.normal(0.0, 1.0, 4000).astype(np.float32)
    _, pav, _ = R.rocch_from_lists(eng, pos, neg)
    assert len(pav.llr) >= 4
    at = np.array([RM.key_score(k) for k in pav.vertices["key"][1:]], np.float32)
    special = np.concatenate([at, np.nextafter(at, np.float32(np.inf)), np.nextafter(at, np.float32(-np.inf)),
                              np.float32([pos.min() - 1, neg.min() - 1, pos.max() + 1, np.inf, -np.inf, np.nan, -np.nan, 0.0, -0.0,
                                          np.finfo(np.float32).max, -np.finfo(np.float32).max])])
    m, nt = 37, 1027                                     # ragged: one whole strip and three columns
    body = rng.normal(0.5, 1.5, (m, nt)).astype(np.float32)
    body.reshape(-1)[:len(special)] = special
    body[-1, -len(special):] = special
    for ld, off in ((1031, 1), (1028, 0)):
        for bound in (0.0, 2.5):
            S = np.full((m, ld), 7.0, np.float32)
            S[:, :nt] = body
            buf = _t(np.concatenate([np.zeros(off, np.float32), S.ravel()]))
            out = torch.full((m * ld + off,), -3.0, dtype=torch.float32, device=_dev())
            torch.cuda.synchronize()
            pav.apply_dev(eng, buf.data_ptr() + 4 * off, ld, m, nt, out.data_ptr() + 4 * off, ld, bound=bound)
            eng.synchronize()
            got = out.cpu().numpy()[off:].reshape(m, ld)
            ref = pav(body, bound)
            assert np.array_equal(got[:, :nt].view(np.uint32), ref.view(np.uint32)), (ld, bound)
            assert np.all(got[:, nt:] == -3.0)                       # columns [Nt, ld_out) are not written
            if bound:
                assert np.nanmax(np.abs(got[:, :nt])) <= bound
            # in place
            pav.apply_dev(eng, buf.data_ptr() + 4 * off, ld, m, nt, bound=bound)
            eng.synchronize()
            inpl = buf.cpu().numpy()[off:].reshape(m, ld)
            assert np.array_equal(inpl[:, :nt].view(np.uint32), ref.view(np.uint32)) and np.all(inpl[:, nt:] == 7.0)
    fin = np.isfinite(body)
    order = np.argsort(body[fin], kind="stable")
    mapped = pav(body)[fin][order]
    assert np.all(mapped[1:] >= mapped[:-1])                       # non-decreasing


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(engines):
    from plda_amd import rocch as R
    from plda_amd import _native as N
    from plda_amd._native import PldaError
    eng = engines[0]
    rng = np.random.default_rng(12)
    m, nt = 40, 1500
    es, ts = rng.integers(0, 9, m), rng.integers(0, 9, nt)
    S = (rng.standard_normal((m, nt)) + 2.0 * (es[:, None] == ts[None, :])).astype(np.float32)
    for bad, n_bad in ((np.nan, 3), (np.inf, 1), (-np.inf, 2)):
        t = S.copy()
        t.reshape(-1)[:n_bad * 7:7] = bad
        with pytest.raises(PldaError, match="%d non-finite" % n_bad) as e:
            _matrix(eng, t, nt, es, ts)
        assert e.value.code == N.PLDA_E_INVAL
    with pytest.raises(PldaError, match="at least one target") as e:
        _matrix(eng, S, nt, es + 1000, ts)                       # no target trial
    assert e.value.code == N.PLDA_E_INVAL
    pos, neg = _split(S, es, ts)
    with pytest.raises(PldaError) as e:
        R.rocch_from_lists(eng, pos, neg[:0])
    assert e.value.code == N.PLDA_E_INVAL
    with pytest.raises(PldaError, match="2 non-finite") as e:
        R.rocch_from_lists(eng, np.concatenate([pos, [np.nan]]), np.concatenate([neg, [np.inf]]))
    assert e.value.code == N.PLDA_E_INVAL
    small = _make(cap=100)                                       # the edge class over a lowered cap: both numbers named
    with pytest.raises(PldaError, match=r"%d trials.* 100" % len(pos)) as e:
        R.rocch_from_lists(small, pos, neg)
    assert e.value.code == N.PLDA_E_CAPACITY and len(pos) > 100
    _check(R.rocch_from_lists(small, pos[:100], neg, points=True), pos[:100], neg, "at the cap")
    # a vertex array too small: PLDA_E_CAPACITY, the needed count in the result
    model = RM.model(pos, neg)
    out = np.zeros(1, R.RESULT_DTYPE)
    verts, llr = np.zeros(2, R.VERTEX_DTYPE), np.zeros(2, np.float64)
    p = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731
    rc = eng._lib.plda_rocch_lists(eng._h, p(pos), len(pos), p(neg), len(neg), 2, p(out), p(verts), p(llr), None, None)
    assert rc == N.PLDA_E_CAPACITY and int(out[0]["n_vertices"]) == len(model["vertices"]) > 2
    assert abs(float(out[0]["min_cllr"]) - model["min_cllr"]) <= 1e-12 and np.all(verts["x"] == 0)
    with pytest.raises(PldaError) as e:
        R.rocch_from_lists(eng, pos, neg, cap_vertices=2)
    assert e.value.code == N.PLDA_E_CAPACITY
    # null pointers
    assert eng._lib.plda_rocch_lists(eng._h, p(pos), len(pos), p(neg), len(neg), 2, None, p(verts), p(llr), None, None) == N.PLDA_E_INVAL
    assert eng._lib.plda_rocch_lists(eng._h, p(pos), len(pos), p(neg), len(neg), 2, p(out), None, p(llr), None, None) == N.PLDA_E_INVAL
    assert eng._lib.plda_rocch_lists(eng._h, None, len(pos), p(neg), len(neg), 2, p(out), p(verts), p(llr), None, None) == N.PLDA_E_INVAL
    dS = _t(S)
    assert eng._lib.plda_rocch_matrix_dev(eng._h, C.c_void_p(dS.data_ptr()), nt, m, nt, None, None, 2, p(out), p(verts), p(llr), None, None) == N.PLDA_E_INVAL
    assert eng._lib.plda_pav_map_dev(eng._h, C.c_void_p(dS.data_ptr()), nt, m, nt, 2, None, p(llr), 0.0, C.c_void_p(dS.data_ptr()), nt) == N.PLDA_E_INVAL
    # more segments than the map's table holds
    big = R.Pav(np.zeros(R.MAX_PAV_VERTICES + 1, R.VERTEX_DTYPE), np.zeros(R.MAX_PAV_VERTICES, np.float64))
    with pytest.raises(PldaError, match="segments") as e:
        big.apply_dev(eng, dS.data_ptr(), nt, m, nt)
    assert e.value.code == N.PLDA_E_CAPACITY
    # the operand form on an unfitted handle
    x = _t(np.zeros((4, 8)))
    ids = _t(np.arange(4, dtype=np.int64))
    with pytest.raises(PldaError, match="not fitted") as e:
        R.rocch_from_operands_dev(eng, x.data_ptr(), None, 1, 4, x.data_ptr(), 4, ids.data_ptr(), ids.data_ptr())
    assert e.value.code == N.PLDA_E_NOT_FITTED
    _check(R.rocch_from_lists(eng, pos, neg, points=True), pos, neg, "after the refusals", model)     # the handle is still usable


# ---------------------------------------------------------------------------------------------- guard bands, poisoned scratch
def _guarded(a, nan, ld=None):
    """`a` inside a buffer with GUARD_BYTES of NaN (or zero; -1 / 0 for integers) on both sides and behind every row."""
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
        buf.fill_(-1 if nan else 0)
    body = buf[g:g + rows * ld].view(rows, ld)[:, :cols]
    body.copy_(t.reshape(rows, cols).to(_dev()))
    torch.cuda.synchronize()
    return buf, body


def _device_cases(eng, nan):
    """The device entry points on guarded inputs -> dict of arrays (the map's output with its guard bands included)."""
    import torch
    from plda_amd import rocch as R
    out = {}
    for m, nt, ld in ((3, 5, 7), (257, 1023, 1030), (1003, 1999, 2004)):
        rng = np.random.default_rng(m + nt)
        es, ts = rng.integers(0, 9, m), rng.integers(0, 9, nt)
        es[0] = ts[0] = 0; ts[-1] = 100
        S = (rng.standard_normal((m, nt)) + 2.0 * (es[:, None] == ts[None, :])).astype(np.float32)
        keep = [_guarded(S, nan, ld), _guarded(es.astype(np.int64), nan), _guarded(ts.astype(np.int64), nan)]
        got = R.rocch_from_matrix_dev(eng, keep[0][1].data_ptr(), ld, m, nt, keep[1][1].data_ptr(), keep[2][1].data_ptr(), points=True)
        if m == 257:
            _check(got, *_split(S, es, ts), "guarded %d x %d" % (m, nt))
        for k, v in _flat(*got).items():
            out["matrix%d_%s" % (m, k)] = v
        obuf, obody = _guarded(np.zeros((m, nt), np.float32), nan, ld)
        before = obuf.clone()
        got[1].apply_dev(eng, keep[0][1].data_ptr(), ld, m, nt, obody.data_ptr(), ld, bound=20.0)
        eng.synchronize()
        mapped = obody.cpu().numpy()
        assert np.array_equal(mapped.view(np.uint32), got[1](S, 20.0).view(np.uint32))
        obody.copy_(torch.zeros_like(obody))
        assert torch.equal(obuf.view(torch.int32), before.view(torch.int32))      # nothing outside the Nt columns was written
        out["map%d" % m] = mapped
    d, m, nt, k = 41, 1003, 1999, 37
    rng = np.random.default_rng(9)
    es, ts = rng.integers(0, k, m), rng.integers(0, k, nt)
    spk = rng.standard_normal((k, d)) * 1.2
    U, V = spk[es] + rng.standard_normal((m, d)), spk[ts] + rng.standard_normal((nt, d))
    n = rng.integers(1, 5, m).astype(np.int32)
    keep = [_guarded(x, nan) for x in (U, V, n, es.astype(np.int64), ts.astype(np.int64))]
    got = R.rocch_from_operands_dev(eng, keep[0][1].data_ptr(), keep[2][1].data_ptr(), 0, m, keep[1][1].data_ptr(), nt,
                                    keep[3][1].data_ptr(), keep[4][1].data_ptr(), points=True)
    for key, v in _flat(*got).items():
        out["operands_%s" % key] = v
    return out


@pytest.mark.parametrize("variant", [0, 2])
def test_device_entry_points_guards_and_poisoned_scratch(variant):
    """Inputs with NaN (or -1) in the 64 KiB before and after them and behind every row, against zero neighbours; then the
    same on poisoned device scratch (PLDA_SCRATCH_POISON=1: every allocation of the library filled with 0xFF bytes): all four
    runs bit-identical."""
    runs = []
    for poison in (False, True):
        for nan in (True, False):
            eng = _make(variant, d=41, slab=256, poison=poison)
            runs.append(_device_cases(eng, nan))
            eng.synchronize()
            del eng
    _make()                                    # the poison switch off again for whatever runs next in this process
    for other in runs[1:]:
        _same_bits(runs[0], other, "guards / poison")


# ---------------------------------------------------------------------------------------------- a long-lived handle
def test_a_long_lived_handle_gives_a_fresh_handles_bits():
    """the new entry points after earlier calls of other entry points (and of themselves at other sizes: large -> small ->
    large) equal a fresh handle's, bit for bit -- the law of tests/test_gpu_handle_history.py"""
    from plda_amd import calibration as CB
    from plda_amd import dcf as DC
    from plda_amd import eer as EE
    from plda_amd import rocch as R
    rng = np.random.default_rng(21)

    def case(m, nt, k):
        es, ts = rng.integers(0, k, m), rng.integers(0, k, nt)
        S = (rng.standard_normal((m, nt)) + 2.0 * (es[:, None] == ts[None, :])).astype(np.float32)
        return _t(S), _t(es.astype(np.int64)), _t(ts.astype(np.int64)), m, nt

    large, small = case(700, 2100, 4), case(9, 130, 3)

    def probe(eng, c):
        import torch
        dS, des, dts, m, nt = c
        got = R.rocch_from_matrix_dev(eng, dS.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr(), points=True)
        out = torch.empty_like(dS)
        got[1].apply_dev(eng, dS.data_ptr(), nt, m, nt, out.data_ptr(), nt)
        eng.synchronize()
        return dict(_flat(*got), map=out.cpu().numpy())

    fresh = {name: probe(_make(), c) for name, c in (("large", large), ("small", small))}
    eng = _make()
    dS, des, dts, m, nt = large
    args = (dS.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr())
    EE.eer_from_matrix_dev(eng, *args)
    DC.min_dcf_from_matrix_dev(eng, *args)
    CB.fit_from_matrix_dev(eng, *args)
    for name, c in (("large", large), ("small", small), ("large", large), ("small", small)):
        _same_bits(probe(eng, c), fresh[name], "long-lived handle, %s" % name)
        DC.min_dcf_from_matrix_dev(eng, *args)
    # and the neighbours still give what they gave: they share no scratch with the hull
    a = DC.min_dcf_from_matrix_dev(eng, *args)
    b = DC.min_dcf_from_matrix_dev(_make(), *args)
    assert a == b


# ---------------------------------------------------------------------------------------------- end to end
def test_end_to_end_plda_min_cllr_and_calibrate_pav():
    from conftest import make_data
    from liblda import PLDA
    x, y = make_data(61, 3000, 32, 60, scale_between=0.15)
    p = PLDA(0)
    p.fit(x, y, 5)
    enrol = p.transform(x[:180], y[:180])                                # 60 models of 3 utterances
    test = p.transform(x[1200:2400], np.arange(1200, dtype=np.uint64))
    test_speaker = {int(i): int(s) for i, s in zip(range(1200), y[1200:2400])}
    p.norm(x[2400:], enrol)
    es = np.array(list(enrol.keys()), np.int64)
    ts = np.array([test_speaker[int(k)] for k in test.keys()], np.int64)
    info = {"t_distinct": 0, "window_start": 0, "window_size": 0, "n_lds": 0, "n_global_atomic": 0, "n_register": 0, "reads": 0}
    for kw, S in (({}, p.score_matrix(enrol, test)), ({"znorm": False}, p.score_matrix(enrol, test, znorm=False))):
        res, pav = p.min_cllr(enrol, test, test_speaker, **kw)           # operand form: the matrix is never held
        pos, neg = _split(S, es, ts)
        _check((res, pav, dict(info, n_lds=max(len(pos), len(neg)))), pos, neg, "PLDA.min_cllr %r" % (kw,))
    cohort = p.transform_array(x[2400:], 1)
    res, pav = p.min_cllr(enrol, test, test_speaker, cohort=cohort, top_k=100)
    pos, neg = _split(p.score_matrix_asnorm(enrol, test, cohort, 100), es, ts)
    _check((res, pav, dict(info, n_lds=max(len(pos), len(neg)))), pos, neg, "PLDA.min_cllr, AS-norm")
    cal = p.calibrate(enrol, test, test_speaker, prior=0.5)
    stored = p.calibrate_pav(enrol, test, test_speaker)
    m = p._instance if hasattr(p, "_instance") else p
    assert m.pav is stored
    S = p.score_matrix(enrol, test)
    pos, neg = _split(S, es, ts)
    floor = RM.model(pos, neg)
    assert [int(v) for v in stored.vertices["key"]] == [v[4] for v in floor["vertices"]]
    print("cllr_after %.17g min_cllr %.17g" % (cal.cllr_after, floor["min_cllr"]))
    assert floor["min_cllr"] <= cal.cllr_after + 1e-12
    mapped = stored(S, bound=60.0).astype(np.float64)
    tgt = es[:, None] == ts[None, :]
    assert abs(RM.cllr_of_llrs(mapped[tgt], mapped[~tgt]) - floor["min_cllr"]) <= 1e-6
    assert np.array_equal(p.score_matrix(enrol, test), S)               # score_matrix and the affine calibration are untouched
