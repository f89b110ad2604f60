"""GPU: the seeded random-shape parity sweep.  tests/sweep_cases.py draws the cases (edge-biased menus, one generator per
module, seeded by (module, seed0, index) alone); every case is one test id `module-index` and is judged by the rule its
module's fixed-case test already uses -- imported from that test, never restated, so no tolerance is introduced here.  The
old hand-run sweeps (scripts/stress_*.py) contribute a committed number of their cases under their own laws.

A failing id prints its case's tag; `sweep_cases.draw(module, index, seed0)` re-creates the case from it.

Hand runs with fresh cases:  PLDA_SWEEP_SEED=<seed0> [PLDA_SWEEP_CASES=<count per module>] pytest -m gpu tests/test_gpu_sweep.py
(the defaults are the committed values: seed0 = 0, sweep_cases.COUNTS and OLD_COUNTS).

Nothing here provokes a fault: every input sits in a buffer the test owns, and no refused input is tried."""
import importlib
import os
import sys

import numpy as np
import pytest

import sweep_cases as sc

pytestmark = pytest.mark.gpu

SEED0 = int(os.environ.get("PLDA_SWEEP_SEED", "0"))
_CASES = os.environ.get("PLDA_SWEEP_CASES")
OLD_COUNTS = {"stress_parity": 8, "stress_parity2": 8, "stress_parity3": 8, "stress_eer": 8, "stress_mixed_counts": 8}
# every creation-time switch an engine of this file may be made under; all are cleared around MPlda(0)
SWITCHES = ("PLDA_SNORM_SLAB_ROWS", "PLDA_SCRATCH_POISON", "PLDA_MIXED_VARIANT", "PLDA_AHC_SCRATCH_BYTES", "PLDA_DER_SCRATCH_BYTES",
            "PLDA_EMBED_VARIANT", "PLDA_GEMM_VARIANT", "PLDA_SCORE_DTYPE", "PLDA_EER_VARIANT", "PLDA_EER_SLAB_ROWS", "PLDA_MINDCF_VARIANT", "PLDA_VBX_SCRATCH_BYTES", "PLDA_ADAPT_SLAB_ROWS", "PLDA_TRANSFORM_VARIANT")


def _count(name, committed):
    return int(_CASES) if _CASES else committed


class _Engines(object):
    """One engine per switch value, made on first use with the switch set and restored around MPlda(0)."""

    def __init__(self):
        self._made = {}

    def get(self, **switches):
        key = tuple(sorted(switches.items()))
        if key not in self._made:
            from plda_amd import MPlda
            saved = {k: os.environ.pop(k, None) for k in SWITCHES}
            try:
                for k, v in switches.items():
                    assert k in SWITCHES, k
                    os.environ[k] = str(v)
                self._made[key] = MPlda(0)
            finally:
                for k in SWITCHES:
                    os.environ.pop(k, None)
                    if saved[k] is not None:
                        os.environ[k] = saved[k]
        return self._made[key]

    def prepared(self, name, make):
        """an engine another test module prepares (`make()`), made once with every switch cleared around it"""
        if name not in self._made:
            saved = {k: os.environ.pop(k, None) for k in SWITCHES}
            try:
                self._made[name] = make()
            finally:
                for k, v in saved.items():
                    if v is not None:
                        os.environ[k] = v
        return self._made[name]


@pytest.fixture(scope="module")
def engines():
    return _Engines()


def _dev():
    import torch
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------- top-N
def _run_topn(case, engines):
    """rule: exact indices and score bits (test_gpu_topn._same) against topn_model.top_n of the crafted matrix, or of the
    matrix score_matrix_dev / score_matrix_snorm_dev writes for the same operands; pieces / slabs by size and of 128 rows"""
    import torch
    import test_gpu_topn as T
    import topn_model as tm
    both = [("default", engines.get()), ("pieces of 128", engines.get(PLDA_SNORM_SLAB_ROWS=128))]
    m, nt = case["m"], case["nt"]
    if case["form"] == "matrix":
        S, ld = case["S"], case["ld"]
        dS = torch.full((m, ld), float("nan"), dtype=torch.float32, device=_dev())       # (a NaN has the highest key of all)
        dS[:, :nt] = T._t(S)
        for axis in (0, 1):
            want = tm.top_n(S, case["top"][axis], axis)
            for name, eng in both:
                T._same("axis %d, %s" % (axis, name), T._matrix_topn(eng, dS, ld, m, nt, axis, case["top"][axis]), want)
        return
    for _, eng in both:
        eng.set_model(*sc.model_params(case["d"], case["model_seed"]))
    U, n, V = case["U"], case["n"], case["V"]
    zn, sn = T._mode_args(case["mode"], case["stats"])
    S = T._full_matrix(both[0][1], U, n, V, zn=zn, sn=sn)
    dS = T._t(S)
    for axis in (0, 1):
        top = case["top"][axis]
        want = tm.top_n(S, top, axis)
        T._same("axis %d matrix form" % axis, T._matrix_topn(both[0][1], dS, nt, m, nt, axis, top), want)
        for name, eng in both:
            T._same("axis %d operand form, %s" % (axis, name), T._operand_topn(eng, U, n, V, axis, top, zn=zn, sn=sn), want)


# ------------------------------------------------------------------------------------------- DER
def _run_der(case, engines):
    """rule: integer equality with der_model.score and the map properties of der_model.check_map (test_gpu_der._check); the
    sweep form against cut + model and cut + der, as test_gpu_der.test_sweep_equals_cut_then_der; the dispatch class asserted"""
    import ahc_model
    import der_model as M
    import test_gpu_der as T
    from plda_amd import der, diarize
    eng = engines.get()
    sr, sh = case["shape"]
    plan = der.plan(eng, sr, sh)
    assert plan["cls"] == case["cls"] and (sr == 0 or plan["lds_max"] == sc.der_lds_max(sr)), (plan, case["cls"])
    offsets = diarize.offsets_of(case["sizes"])
    ref, dur = case["ref"], case["dur"]
    cut_at = lambda a, q: None if a is None else a[int(offsets[q]):int(offsets[q + 1])]      # noqa: E731
    if case["form"] == "der":
        recs = [(cut_at(ref, q), cut_at(case["hyp"], q), cut_at(dur, q)) for q in range(len(case["sizes"]))]
        counts, mp = T._check(eng, recs, case["tag"])
        small = engines.get(PLDA_DER_SCRATCH_BYTES=1 << 20)
        c2, m2 = T._check(small, recs, case["tag"] + " (scratch budget of 1 MiB)")
        assert np.array_equal(counts, c2) and np.array_equal(mp, m2)
        return
    labels, ncl, merges = diarize.ahc(eng, case["blocks"], None, 1, return_merges=True)
    import test_gpu_ahc as TA
    TA._assert_equal((labels, ncl) + merges, ahc_model.cluster(case["blocks"], None, 1), "the merge record")
    ns, thresholds = case["num_speakers"], case["thresholds"]
    counts, k = T._run_sweep(eng, merges, offsets, ref, thresholds, dur, ns)
    for q, thr in enumerate(thresholds):
        hyp, kq = diarize.cut(merges, offsets, float(thr), ns)
        assert np.array_equal(k[q], kq), "n_clusters at threshold %d" % q
        assert np.array_equal(counts[q], M.score(ref, hyp, offsets, dur)), "counts at threshold %d against cut + model" % q
        assert np.array_equal(counts[q], der.der(eng, ref, hyp, offsets, dur).counts), "counts at threshold %d against cut + der" % q
    if len(thresholds) > 2:
        assert np.array_equal(counts[0], counts[-1]) and np.array_equal(k[0], k[-1])         # the two equal thresholds


# ------------------------------------------------------------------------------------------- AHC
def _run_ahc(case, engines):
    """rule: bit equality of all five outputs with ahc_model.cluster (test_gpu_ahc._assert_equal); the operand form against
    the matrix form and the model on the blocks score_matrix_dev writes; a scratch budget of 1 MiB changes nothing"""
    import torch
    import ahc_model as M
    import test_gpu_ahc as T
    from plda_amd import diarize
    eng, small = engines.get(), engines.get(PLDA_AHC_SCRATCH_BYTES=1 << 20)
    assert diarize.plan(eng, 1)["lds_max"] == sc.AHC_LDS_MAX
    if case["form"] == "matrix":
        blocks = case["blocks"]
    else:
        eng.set_model(*T._model_params(case["d"], case["model_seed"]))
        offsets = diarize.offsets_of(case["sizes"])
        dX = torch.from_numpy(case["vecs"]).to(_dev())
        blocks = T._scored_blocks(eng, dX, offsets)
    thr, ns = sc.ahc_stop(case, M.cluster(blocks[:1], None, 1)[4])
    want = M.cluster(blocks, thr, ns)
    T._assert_equal(T._run(eng, blocks, thr, ns), want, "matrix form")
    T._assert_equal(T._run(small, blocks, thr, ns), want, "matrix form, scratch budget of 1 MiB")
    if case["form"] == "operand":
        T._assert_equal(T._run_operands(eng, dX, offsets, thr, ns), want, "operand form")


# ------------------------------------------------------------------------------------------- AS-norm cohort statistics
def _run_asnorm(case, engines):
    """rule: test_gpu_asnorm._check_exact on the fp32 scores score_matrix_dev writes for the same operands; bit-identical
    between two calls and between slab heights"""
    import test_gpu_asnorm as T
    eng, small = engines.get(), engines.get(PLDA_SNORM_SLAB_ROWS=128)
    for e in (eng, small):
        e.set_model(*sc.model_params(case["d"], case["model_seed"]))
    X, n, Cv, K = case["X"], case["n"], case["Cv"], case["K"]
    S32 = T._scores(eng, X, n, Cv)
    mean, std = T._stats(eng, X, n, Cv, K)
    T._check_exact(case["tag"], S32, K, mean, std)
    again = T._stats(eng, X, n, Cv, K)
    assert np.array_equal(mean, again[0]) and np.array_equal(std, again[1])            # two calls: bit-identical
    m2, s2 = T._stats(small, X, n, Cv, K)
    assert np.array_equal(mean, m2) and np.array_equal(std, s2)                        # slabs of 128 rows: bit-identical


# ------------------------------------------------------------------------------------------- the labelled-trials consumers
def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _trials_on_device(case):
    """(device buffer, pointer of the matrix `off` floats into it, enrol speakers, test speakers)"""
    import torch
    off = case["off"]
    dS = _t(np.concatenate([np.zeros(off, np.float32), case["S"].ravel()]))
    des, dts = _t(case["es"]), _t(case["ts"])
    torch.cuda.synchronize()
    return dS, dS.data_ptr() + 4 * off, des, dts


def _operands_on_device(case, eng):
    """the operands of rule B and the fp32 matrix score_matrix_dev writes for them"""
    import torch
    eng.set_model(*sc.model_params(case["d"], case["model_seed"]))
    m, nt, n, z = case["m"], case["nt"], case["n"], case["z"]
    dU, dV, des, dts = _t(case["U"]), _t(case["V"]), _t(case["es"]), _t(case["ts"])
    dn, nu = (None, int(n)) if np.isscalar(n) else (_t(n), 0)
    dzm, dzs = (_t(z[0]), _t(z[1])) if z is not None else (None, None)
    S = torch.empty((m, nt), dtype=torch.float32, device=_dev())
    torch.cuda.synchronize()
    eng.score_matrix_dev(dU.data_ptr(), _ptr(dn), nu, m, dV.data_ptr(), nt, S.data_ptr(), nt, _ptr(dzm), _ptr(dzs))
    eng.synchronize()
    return dict(dU=dU, dV=dV, des=des, dts=dts, dn=dn, nu=nu, dzm=dzm, dzs=dzs, S=S)


def _run_mindcf(case, engines):
    """rule A: bit equality with mindcf_model.model (test_gpu_mindcf._assert_same) under every PLDA_MINDCF_VARIANT arm, and
    the EER of the same trials against the restatement (test_gpu_eer._assert_matrix_eer); rule B: the matrix form, the list
    form and the operand form (slabs of 256 rows, 257 or 513 rows) give one answer"""
    import mindcf_model as mm
    import test_gpu_eer as TE
    import test_gpu_mindcf as T
    from oracle import plda_oracle_np as onp
    from plda_amd import dcf, eer
    pts = mm.FIVE if case["points"] == "five" else mm.NIST
    m, nt, es, ts = case["m"], case["nt"], case["es"], case["ts"]
    tgt = es[:, None] == ts[None, :]
    if case["form"] == "matrix":
        dS, ptr, des, dts = _trials_on_device(case)
        sub = case["S"][:, :nt]
        pos, neg = mm.split(sub, es, ts)
        ref = mm.model(pos, neg, pts)
        for variant in (0, 1, 2):
            eng = engines.get(PLDA_MINDCF_VARIANT=variant) if variant else engines.get()
            got, info = dcf.min_dcf_from_matrix_dev(eng, ptr, case["ld"], m, nt, des.data_ptr(), dts.data_ptr(), pts)
            T._assert_same(got, ref, "matrix variant %d" % variant)
            assert (info["Np"], info["Nn"]) == (len(pos), len(neg))
            lst, _ = dcf.min_dcf_from_lists(eng, pos, neg, pts)
            T._assert_same(lst, ref, "lists variant %d" % variant)
        eref = onp.eer(neg, pos)
        for variant in (0, 1, 2):
            eng = engines.get(PLDA_EER_VARIANT=variant) if variant else engines.get()
            TE._assert_matrix_eer(eer.eer_from_matrix_dev(eng, ptr, case["ld"], m, nt, des.data_ptr(), dts.data_ptr()), eref, tgt)
        return
    eng = engines.get(PLDA_EER_SLAB_ROWS=sc.OPERAND_SLAB_ROWS)
    o = _operands_on_device(case, eng)
    pos, neg = mm.split(o["S"].cpu().numpy(), es, ts)
    ref = mm.model(pos, neg, pts)
    mat, _ = dcf.min_dcf_from_matrix_dev(eng, o["S"].data_ptr(), nt, m, nt, o["des"].data_ptr(), o["dts"].data_ptr(), pts)
    args = (o["dU"].data_ptr(), _ptr(o["dn"]), o["nu"], m, o["dV"].data_ptr(), nt, o["des"].data_ptr(), o["dts"].data_ptr(), _ptr(o["dzm"]), _ptr(o["dzs"]))
    opr, _ = dcf.min_dcf_from_operands_dev(eng, *args, pts)
    opr2, _ = dcf.min_dcf_from_operands_dev(eng, *args, pts)
    lst, _ = dcf.min_dcf_from_lists(eng, pos, neg, pts)
    T._assert_same(mat, ref, "matrix form")
    T._assert_same(lst, ref, "list form")
    T._assert_same(opr, ref, "operand form, slabs of 256 rows")
    T._assert_same(opr, mat, "operand form against matrix form")
    T._assert_same(opr2, opr, "operand form again")
    for variant in (1, 2):                       # the EER without the matrix: the three-pass form and the single pass forced
        e2 = engines.get(PLDA_EER_SLAB_ROWS=sc.OPERAND_SLAB_ROWS, PLDA_EER_VARIANT=variant)
        e2.set_model(*sc.model_params(case["d"], case["model_seed"]))
        want = eer.eer_from_matrix_dev(e2, o["S"].data_ptr(), nt, m, nt, o["des"].data_ptr(), o["dts"].data_ptr())
        TE._assert_matrix_eer(want, onp.eer(neg, pos), tgt)
        assert np.array_equal(eer.eer_from_operands_dev(e2, *args), want), "EER operand form, variant %d" % variant


# ------------------------------------------------------------------------------------------- calibration
def _run_calibration(case, engines):
    """rule A: the pass record against calibration_model under test_gpu_calibration._compare, bit-identical between two
    calls; the fit under the optimality rule (_assert_fit_is_optimal) and the equivariance check (_assert_equivariant);
    rule B: matrix, list and operand forms (slabs of 256 rows) against the model's record of the device's own scores"""
    import calibration_model as cm
    import test_gpu_calibration as T
    from plda_amd import calibration as CB
    m, nt, es, ts = case["m"], case["nt"], case["es"], case["ts"]
    if case["form"] == "operand":
        eng = engines.get(PLDA_EER_SLAB_ROWS=sc.OPERAND_SLAB_ROWS)
        o = _operands_on_device(case, eng)
        Sh = o["S"].cpu().numpy()
        pos, neg = cm.split(Sh, es, ts)
        for a, c, theta in case["passes"]:
            ref = cm.pass_matrix(Sh, es, ts, a, c, theta)
            mat = CB.pass_from_matrix_dev(eng, o["S"].data_ptr(), nt, m, nt, o["des"].data_ptr(), o["dts"].data_ptr(), a, c, theta)
            lst = CB.pass_from_lists(eng, pos, neg, a, c, theta)
            opr = CB.pass_from_operands_dev(eng, o["dU"].data_ptr(), _ptr(o["dn"]), o["nu"], m, o["dV"].data_ptr(), nt, o["des"].data_ptr(),
                                            o["dts"].data_ptr(), _ptr(o["dzm"]), _ptr(o["dzs"]), a, c, theta)
            for what, got in (("matrix", mat), ("lists", lst), ("operands, slabs of 256 rows", opr)):
                T._compare("%s at (%.3g, %.3g)" % (what, a, c), got, ref)
        return
    eng = engines.get()
    dS, ptr, des, dts = _trials_on_device(case)
    sub = case["S"][:, :nt]
    pos, neg = cm.split(sub, es, ts)
    if case["form"] == "pass":
        for a, c, theta in case["passes"]:
            got = CB.pass_from_matrix_dev(eng, ptr, case["ld"], m, nt, des.data_ptr(), dts.data_ptr(), a, c, theta)
            again = CB.pass_from_matrix_dev(eng, ptr, case["ld"], m, nt, des.data_ptr(), dts.data_ptr(), a, c, theta)
            for key in got:
                assert np.asarray(got[key]).tobytes() == np.asarray(again[key]).tobytes(), key
            ref = cm.pass_matrix(sub, es, ts, a, c, theta)
            T._compare("matrix at (%.3g, %.3g)" % (a, c), got, ref)
            T._compare("lists at (%.3g, %.3g)" % (a, c), CB.pass_from_lists(eng, pos, neg, a, c, theta), ref)
        return
    prior, k, d, tol = case["prior"], case["k"], case["d"], 1e-18
    fm = CB.fit_from_matrix_dev(eng, ptr, case["ld"], m, nt, des.data_ptr(), dts.data_ptr(), prior)
    fl = CB.fit_from_lists(eng, pos, neg, prior, tol, 100)
    for what, f in (("matrix", fm), ("lists", fl)):
        T._assert_fit_is_optimal(what, f, pos, neg, prior, tol)
    f2 = CB.fit_from_lists(eng, sc.shifted(pos, k, d), sc.shifted(neg, k, d), prior, tol, 100)
    T._assert_equivariant(fl, f2, k, d)


# ------------------------------------------------------------------------------------------- embedding chain
def _run_embed(case, engines):
    """rule: the a-priori bound ratio <= 1 (test_gpu_embed._ratio) and bits that do not depend on the batch (_same); the
    dispatch class asserted through plda_embed_plan"""
    import test_gpu_embed as T
    eng = engines.get(PLDA_EMBED_VARIANT=1) if case["forced"] else engines.get()
    ch, x = case["chain"], case["x"]
    try:
        eng.set_embedding(T._chain(ch))
        has_a = ch.A is not None
        assert T._plan(eng, case["din"], case["dout"] if has_a else case["din"], has_a, int(x.dtype == np.float32))[0] == case["cls"]
        full = eng.embed(x)
        ratio = T._ratio(full, ch, x)
        print("%.3f of the bound" % ratio)
        assert ratio <= 1.0, ratio
        assert T._same(full, eng.embed(x)), "run to run"
        r = x.shape[0]
        for i in sorted({0, r // 2, r - 1}):
            assert T._same(full[i:i + 1], eng.embed(x[i:i + 1])), "row %d alone" % i
        idx = np.random.default_rng(r).permutation(r)[:max(1, r // 2)]
        assert T._same(full[idx], eng.embed(x[idx])), "inside a smaller batch at other positions"
    finally:
        eng.set_embedding(None)


# ------------------------------------------------------------------------------------------- VBx
def _run_vbx(case, engines):
    """rule: the bands of test_gpu_vbx.test_parity_with_the_model (_assert_parity) per recording; the plan class asserted; a
    scratch budget of 1 MiB gives the same bits"""
    import test_gpu_vbx as T
    eng = engines.prepared("vbx", T._engine)
    small = engines.get(PLDA_VBX_SCRATCH_BYTES=1 << 20)
    small.set_model(*T._model(4))
    got = T._run(eng, case["recs"], case["phi"], case["params"])
    for q, ((y, labels), (want, ld)) in enumerate(zip(case["recs"], case["refs"])):
        T._assert_parity(got, want, ld, len(labels), q)
        assert T.plan_class(eng, len(labels), int(labels.max()) + 1, case["d"]) == case["classes"][q]
    T._assert_same(T._run(small, case["recs"], case["phi"], case["params"]), got, "1 MiB budget")


# ------------------------------------------------------------------------------------------- adaptation
def _run_adapt(case, engines):
    """rule: the record within its bound of the model's (test_gpu_adapt._assert_record), bit-identical between two calls
    (_same), the same within the bound in pieces over slabs of 64 rows and merged with adapt_add_stats; the update and the
    blend against adapt_model under _assert_model"""
    import adapt_model as AM
    import test_gpu_adapt as T
    eng, small = engines.get(), engines.get(PLDA_ADAPT_SLAB_ROWS=64)
    model, x, w = case["model"], case["x"], case["w"]
    mean = model[0]
    for e in (eng, small):
        e.set_model(*model)
        e.adapt_reset()
    eng.adapt_accumulate(x, w)
    one = eng.adapt_stats()
    T._assert_record(one, AM.record(x, mean, w), x, mean, w)
    eng.adapt_reset()
    eng.adapt_accumulate(x, w)
    assert T._same([T._aug(one)], [T._aug(eng.adapt_stats())])                 # the same call twice: bit-identical
    bound = 1e-12 * AM.record_bound(x, mean, w)
    cuts = case["pieces"]
    parts = [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    for a, b in parts:                                                        # one call in pieces, slabs of 64 rows
        small.adapt_accumulate(x[a:b], None if w is None else w[a:b])
    pieces = small.adapt_stats()
    assert pieces["rows"] == x.shape[0] and (np.abs(T._aug(pieces) - T._aug(one)) <= bound).all()
    if len(parts) > 1:                                                        # two handles merged through adapt_add_stats
        a, b = parts[0]
        for e, (lo, hi) in ((eng, (a, b)), (small, (b, x.shape[0]))):
            e.adapt_reset()
            e.adapt_accumulate(x[lo:hi], None if w is None else w[lo:hi])
        s2 = small.adapt_stats()
        eng.adapt_add_stats(s2["tot_weight"], s2["rows"], s2["pilot"], s2["s1"], s2["s2"])
        merged = eng.adapt_stats()
        assert merged["rows"] == x.shape[0] and (np.abs(T._aug(merged) - T._aug(one)) <= bound).all()
    eng.set_model(*model)
    eng.adapt(x, w, *case["scales"])
    T._assert_model(eng.get_model(), AM.update_kaldi(mean, model[1], model[2], AM.record(x, mean, w), *case["scales"]))
    eng.set_model(*model)
    eng.blend(case["other"], case["alpha"], case["alpha_mean"])
    T._assert_model(eng.get_model(), AM.blend(model, case["other"], case["alpha"], case["alpha_mean"]))


# ------------------------------------------------------------------------------------------- fusion
def _run_fusion(case, engines):
    """rule A: the pass record against fusion_model under test_gpu_fusion._compare, bit-identical between two calls; the fit
    under the optimality rule (_assert_fit_is_optimal); rule B: the matrices and the lists give one answer"""
    import fusion_model as fm
    import test_gpu_fusion as T
    from plda_amd import fusion as FU
    eng = engines.get()
    S, m, nt, k, es, ts = case["systems"], case["m"], case["nt"], case["k"], case["es"], case["ts"]
    P = T.Placed(S, case["lds"], case["offs"])
    des, dts = _t(es), _t(ts)
    pos, neg = fm.split(S, es, ts)
    if case["form"] == "pass":
        a, c = case["a"], case["c"]
        theta = T._theta(S, a, c)
        got = FU.pass_from_matrices_dev(eng, P.ptrs, P.lds, m, nt, des.data_ptr(), dts.data_ptr(), a, c, theta)
        T._same_bits(got, FU.pass_from_matrices_dev(eng, P.ptrs, P.lds, m, nt, des.data_ptr(), dts.data_ptr(), a, c, theta))
        ref = fm.pass_record(pos, neg, a, c, theta)
        T._compare("matrices", got, ref)
        lst = FU.pass_from_lists(eng, pos, neg, a, c, theta)
        T._compare("lists", lst, ref)
        for key in T.INTS:
            assert lst[key] == got[key]
    else:
        prior = case["prior"]
        T._assert_fit_is_optimal(FU.fit_from_matrices_dev(eng, P.ptrs, P.lds, m, nt, des.data_ptr(), dts.data_ptr(), prior), pos, neg, k, prior)
        T._assert_fit_is_optimal(FU.fit_from_lists(eng, pos, neg, prior, 1e-18, 100), pos, neg, k, prior)
    assert P.unchanged()


# ------------------------------------------------------------------------------------------- transform
def _run_transform(case, engines):
    """rule: test_gpu_transform_edges' (transform_model.assert_rule on one copy per launch and pool entry, all copies of an entry
    inside a launch bit-identical); the arm and the launches asserted through plda_transform_plan"""
    import test_gpu_transform_edges as T
    import transform_model as M
    eng = engines.get(PLDA_TRANSFORM_VARIANT=1) if case["arm"] == "pair" else engines.get()
    pool = T._Pool(case["model"], case["x"], case["n"], case["form"], case["uniform"])
    eng.set_model(*case["model"])
    p1 = eng.transform_plan(1)
    pair = case["arm"] == "pair" or case["dout"] > 512
    assert p1["arm"] == ("pair" if pair else "fused")
    r = sc.transform_rows(case["rows"], p1["cus"], p1["main_block"] if not pair else 128)
    fig, plan = pool.run(eng, r, case["tag"], seed=case["index_seed"])
    assert M.shapes_of(plan) == ({("main", 4)} if pair else sc.transform_shapes(case["rows"], p1["main_block"])), plan
    print("deviation %.3g B, residual %.2f u" % (fig["dev"], fig["rho"]))


RUNNERS = {"topn": _run_topn, "transform": _run_transform, "der": _run_der, "ahc": _run_ahc, "asnorm": _run_asnorm, "mindcf": _run_mindcf, "calibration": _run_calibration, "embed": _run_embed, "vbx": _run_vbx, "adapt": _run_adapt, "fusion": _run_fusion}
assert sorted(RUNNERS) == sorted(sc.MODULES)
_IDS = [(m, i) for m in sc.MODULES for i in range(_count(m, sc.COUNTS[m]))]


def _stop_on_a_device_fault(text):
    """A device fault ends the whole sweep at once: nothing more is started on a device that has faulted."""
    if any(w in text for w in ("illegal memory access", "hipErrorIllegalAddress", "hipErrorLaunchFailure", "unspecified launch failure")):
        pytest.exit("device fault, the sweep stops here: " + text[:300], returncode=3)


@pytest.mark.parametrize("module,index", _IDS, ids=["%s-%d" % mi for mi in _IDS])
def test_sweep(engines, module, index):
    case = sc.draw(module, index, SEED0)
    print(case["tag"])
    try:
        RUNNERS[module](case, engines)
    except Exception as e:      # noqa: BLE001
        _stop_on_a_device_fault(repr(e))
        raise


# ------------------------------------------------------------------------------------------- the old sweeps, their own laws
_OLD = [(s, i) for s in sorted(OLD_COUNTS) for i in range(_count(s, OLD_COUNTS[s]))]
_SCRIPTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts")


@pytest.fixture(scope="module")
def eer_engines():
    return _script("stress_eer").make_engines()


def _script(name):
    if _SCRIPTS not in sys.path:
        sys.path.insert(0, _SCRIPTS)
    return importlib.import_module(name)


@pytest.mark.parametrize("script,index", _OLD, ids=["%s-%d" % si for si in _OLD])
def test_old_sweep(request, script, index):
    """scripts/<script>.py::run_case(index, seed0): the loop body of the hand-run sweep, with the script's own tolerances"""
    kw = {"engines": request.getfixturevalue("eer_engines")} if script == "stress_eer" else {}
    try:
        fails = _script(script).run_case(index, SEED0, **kw)
    except Exception as e:      # noqa: BLE001
        _stop_on_a_device_fault(repr(e))
        raise
    _stop_on_a_device_fault(repr(fails))
    assert not fails, "%s case %d seed0 %d: %s" % (script, index, SEED0, fails)
