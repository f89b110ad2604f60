"""CPU: the laws of the sweep's case generators (tests/sweep_cases.py), so that the device sweep (tests/test_gpu_sweep.py) means
what it says:

  determinism      two draws of one (module, index, seed0) are bit-identical, and independent of what was drawn before;
  coverage         at seed0 = 0 and the committed counts every entry of every menu -- sizes, contents, forms, dispatch classes --
                   is hit at least once per module (nobody can shrink a menu's reach by shrinking a count);
  well-posedness   at most 10 % of a module's draws were re-drawn because the host model found them ill-posed;
  power            per module one planted mutant of the HOST MODEL is rejected, by the module's own comparison rule, on at
                   least one committed case: a sweep whose cases cannot tell the mutant from the model is not doing its job."""
import numpy as np
import pytest

import sweep_cases as sc


def _flat(v, out):
    if isinstance(v, dict):
        for k in sorted(v, key=str):
            out.append(str(k).encode())
            _flat(v[k], out)
    elif isinstance(v, (list, tuple)):
        out.append(b"[%d" % len(v))
        for x in v:
            _flat(x, out)
    elif isinstance(v, np.ndarray) and v.dtype == np.longdouble:       # (its bytes hold padding: head and tail as doubles)
        head = v.astype(np.float64)
        _flat([head, (v - head).astype(np.float64)], out)
    elif isinstance(v, np.ndarray):
        out.append(str((v.dtype, v.shape)).encode())
        out.append(np.ascontiguousarray(v).tobytes())
    elif hasattr(v, "__dict__") and not callable(v):
        _flat(vars(v), out)
    else:
        out.append(repr(v).encode())
    return out


def _bits(case):
    return b"|".join(_flat(case, []))


_COMMITTED = {}


def _committed(module):
    if module not in _COMMITTED:
        _COMMITTED[module] = sc.cases(module)
    return _COMMITTED[module]


def test_counts_meet_the_floor():
    assert sorted(sc.COUNTS) == sorted(sc.MODULES) == sorted(sc.MENUS)
    assert all(sc.COUNTS[m] >= 24 for m in sc.MODULES)


@pytest.mark.parametrize("module", sc.MODULES)
def test_draws_are_deterministic(module):
    first = _committed(module)
    for index in (sc.COUNTS[module] - 1, 0, 17, 5):             # out of order, after everything else was drawn
        again = sc.draw(module, index, 0)
        assert again["tag"] == first[index]["tag"]
        assert _bits(again) == _bits(first[index]), first[index]["tag"]
    other = sc.draw(module, 5, 1)
    assert other["tag"] != first[5]["tag"] and _bits(other) != _bits(first[5])
    assert all(c["tag"].startswith("%s-%d seed0=0" % (module, i)) for i, c in enumerate(first))


@pytest.mark.parametrize("module", sc.MODULES)
def test_committed_cases_hit_every_menu_entry(module):
    hit = {name: set() for name in sc.MENUS[module]}
    for c in _committed(module):
        assert set(c["hits"]) <= set(hit), c["tag"]
        for name, entry in c["hits"].items():
            assert entry in sc.MENUS[module][name], (c["tag"], name, entry)
            hit[name].add(entry)
    missing = {name: sorted(set(sc.MENUS[module][name]) - got, key=str) for name, got in hit.items() if set(sc.MENUS[module][name]) - got}
    assert not missing, "%s: %d cases leave menu entries unhit: %r" % (module, sc.COUNTS[module], missing)


@pytest.mark.parametrize("module", sc.MODULES)
def test_at_most_a_tenth_of_the_draws_is_redrawn(module):
    cases = _committed(module)
    redrawn = sum(1 for c in cases if c["redraws"])
    assert redrawn <= 0.10 * len(cases), "%s: %d of %d draws were ill-posed" % (module, redrawn, len(cases))


# ------------------------------------------------------------------------------------------- power: one mutant per module
def _rejects(rule, *args):
    try:
        rule(*args)
    except AssertionError:
        return True
    return False


def _topn_mutant(S32, n, axis):
    """topn_model.top_n with a tie going to the LARGER index"""
    import topn_model as tm
    lines = np.ascontiguousarray(S32 if axis == 0 else S32.T)
    key = tm.score_key(lines).astype(np.int64)
    index = (lines.shape[1] - 1 - np.argsort(-key[:, ::-1], axis=1, kind="stable"))[:, :n].astype(np.int64)
    return np.take_along_axis(lines.view(np.uint32), index, axis=1).view(np.float32), index


def _power_topn(case):
    import topn_model as tm
    from test_gpu_topn import _same
    if case["form"] != "matrix":
        return False
    return any(_rejects(_same, "mutant", _topn_mutant(case["S"], case["top"][axis], axis), tm.top_n(case["S"], case["top"][axis], axis))
               for axis in (0, 1))


def _greedy_assign(C):
    """der_model.assign with the largest cell first instead of the optimum"""
    C = np.array(C, dtype=object)
    weight = 0
    if C.size:
        C = C.copy()
        while True:
            i, j = divmod(int(np.argmax(C)), C.shape[1])
            if C[i, j] <= 0:
                break
            weight += int(C[i, j])
            C[i, :] = -1
            C[:, j] = -1
    return weight, [-1] * C.shape[0]


def _power_der(case, monkeypatch):
    import der_model as M
    from plda_amd import diarize
    if case["form"] != "der":
        return False
    offsets = diarize.offsets_of(case["sizes"])
    want = M.score(case["ref"], case["hyp"], offsets, case["dur"])
    with monkeypatch.context() as mp:
        mp.setattr(M, "assign", _greedy_assign)
        got = M.score(case["ref"], case["hyp"], offsets, case["dur"])
    return not np.array_equal(got, want)                     # (the rule of test_gpu_der._check: counts are ==)


def _ahc_mutant_one(S, threshold=None, min_clusters=1):
    """ahc_model.cluster_one_definition with a tie going to the LARGER partner b of the same a"""
    import ahc_model as M
    sums = M.costs(S)
    n = sums.shape[0]
    size, alive, slot_of = np.ones(n, np.int64), np.ones(n, bool), np.arange(n)
    upper = np.triu(np.ones((n, n), bool), 1)
    merges = []
    k = n
    while k > 1:
        V = np.where(upper & alive[:, None] & alive[None, :], sums / (size[:, None] * size[None, :]).astype(np.float64), np.inf)
        a = int(np.argmin(V)) // n
        v = V[a].min()
        b = int(np.nonzero(V[a] == v)[0][-1])
        if M._stops(k, v, threshold, min_clusters):
            break
        merges.append((a, b, v))
        x = alive.copy()
        x[a] = x[b] = False
        sums[a, x] = sums[a, x] + sums[b, x]
        sums[x, a] = sums[a, x]
        size[a] += size[b]
        alive[b] = False
        slot_of[slot_of == b] = a
        k -= 1
    return M._finish(n, slot_of, merges)


def _power_ahc(case):
    import ahc_model as M
    from test_gpu_ahc import _assert_equal
    if case["form"] != "matrix":
        return False
    thr, ns = sc.ahc_stop(case, M.cluster(case["blocks"][:1], None, 1)[4])
    return _rejects(_assert_equal, M.cluster(case["blocks"], thr, ns, one=_ahc_mutant_one), M.cluster(case["blocks"], thr, ns))


def test_an_asnorm_case_overflows_a_wave_share():
    """the cap-overflow path of csrc/snorm.hip: on the model's scores of a committed case, a compaction attempt with at most
    GATE candidates of which more than WCAP sit in one wave's share (asnorm_model.compaction_attempts restates the shares)"""
    import asnorm_model as am
    from oracle import plda_oracle_np as onp
    hit = []
    for case in _committed("asnorm"):
        if case["Cv"].shape[0] <= 16 * am.WCAP:
            continue
        psi = sc.model_params(case["d"], case["model_seed"])[2]
        S32 = onp.llr_matrix(psi, case["X"], case["n"], case["Cv"]).astype(np.float32)
        tries = [t for row in S32 for t in am.compaction_attempts(row, case["K"])]
        if any(cand <= am.GATE and per > am.WCAP for _, cand, per in tries):
            assert any(per <= am.WCAP for _, _, per in tries)             # ... and a later level then fits
            hit.append(case["tag"])
    print("cap overflow on %d cases: %s" % (len(hit), hit))
    assert hit


def _power_asnorm(case):
    """K - 1 values instead of K, on host scores of the case's operands (the device test takes the device's)"""
    import asnorm_model as am
    from oracle import plda_oracle_np as onp
    from test_gpu_asnorm import _check_exact
    K = case["K"]
    if K < 2:
        return False
    psi = sc.model_params(case["d"], case["model_seed"])[2]
    S32 = onp.llr_matrix(psi, case["X"], case["n"], case["Cv"]).astype(np.float32)
    mean, std = am.topk_stats(S32, K)
    _check_exact("the model", S32, K, mean, std)
    return _rejects(_check_exact, "the mutant", S32, K, *am.topk_stats(S32, K - 1))


def _mindcf_mutant(pos, neg, points):
    """mindcf_model.model with `>` for `>=` at the threshold on the target side: a target AT the cut's key is not a miss"""
    import mindcf_model as mm
    kp, kn = np.sort(mm.keys(pos)), np.sort(mm.keys(neg))
    allk = np.unique(np.concatenate([kp, kn]))
    miss = np.concatenate([[0], np.searchsorted(kp, allk, side="left")])
    fa = np.concatenate([[len(kn)], len(kn) - np.searchsorted(kn, allk, side="right")])
    out = []
    for pt in points:
        v = mm.value(pt, miss, fa, len(kp), len(kn))
        i = int(np.argmin(v))
        out.append(mm._report(pt, v[i], miss[i], fa[i], len(kp), len(kn), i, allk))
    return out


def _power_mindcf(case):
    import mindcf_model as mm
    if case["form"] != "matrix":
        return False
    pts = mm.FIVE if case["points"] == "five" else mm.NIST
    pos, neg = mm.split(case["S"][:, :case["nt"]], case["es"], case["ts"])
    return not all(mm.same(g, r) for g, r in zip(_mindcf_mutant(pos, neg, pts), mm.model(pos, neg, pts)))   # (test_gpu_mindcf._assert_same)


def _power_calibration(case):
    """the Hessian term sum w s dropped from the non-target class of the pass record"""
    import calibration_model as cm
    from test_gpu_calibration import _compare
    if case["form"] != "pass":
        return False
    a, c, theta = case["passes"][0]
    ref = cm.pass_matrix(case["S"][:, :case["nt"]], case["es"], case["ts"], a, c, theta)
    _compare("the model", ref, ref)
    return _rejects(_compare, "the mutant", dict(ref, H1_n=0.0), ref)


def _power_embed(case):
    """length-normalisation BEFORE centring"""
    import embed_model as em
    from test_gpu_embed import _ratio
    ch, x = case["chain"], case["x"]
    first = em.apply(em.Chain(None, ch.len_in, None, None, 0.0), x)
    mutant = em.apply(em.Chain(ch.m_in, 0.0, ch.A, ch.m_out, ch.len_out), first)
    assert _ratio(em.apply(ch, x), ch, x) <= 1.0
    return not _ratio(mutant, ch, x) <= 1.0


def _vbx_mutant(y, labels, phi, fa, fb, loop_prob, max_iters):
    """vbx_model.run (epsilon = -inf) with the (1 - P) pi re-entry term dropped from the forward pass"""
    import vbx_model as M
    f = np.float64
    y, phi, rho, g, gamma, pi = M._start(y, labels, phi, 5.0, f)
    t, s = gamma.shape
    p = f(loop_prob)
    elbo, max_lp = [], 0.0
    for i in range(max_iters):
        lp, reg = M._emission(gamma, rho, phi, g, f(fa), f(fb))
        max_lp = max(max_lp, float(np.max(np.abs(lp))))
        m = lp.max(axis=1)
        b = np.exp(lp - m[:, None])
        a, c, beta = np.empty((t, s), f), np.empty(t, f), np.empty((t, s), f)
        u = b[0] * pi
        c[0] = u.sum()
        a[0] = u / c[0]
        for j in range(1, t):
            u = b[j] * (p * a[j - 1])                        # <- the mutation
            c[j] = u.sum()
            a[j] = u / c[j]
        beta[t - 1] = 1
        for j in range(t - 2, -1, -1):
            w = b[j + 1] * beta[j + 1]
            beta[j] = (p * w + (1 - p) * np.sum(pi * w)) / c[j + 1]
        gamma = a * beta
        pin = gamma[0] + (1 - p) * pi * np.sum(b[1:] * beta[1:] / c[1:, None], axis=0)
        pi = pin / pin.sum()
        elbo.append(np.sum(np.log(c)) + np.sum(m) + reg)
    return M._finish(gamma, pi, elbo, len(elbo), max_iters, max_lp)


def _power_vbx(case):
    import vbx_model as M
    from test_gpu_vbx import _assert_parity
    (y, labels), (want, ld) = case["recs"][0], case["refs"][0]
    if len(labels) < 2 or int(labels.max()) < 1 or case["params"][2] == 0.0:
        return False                                         # (one segment, one speaker, or P = 0: the term is absent or all there is)
    as_run = lambda r: {"gamma": [r["gamma"]], "pi": [r["pi"]], "elbo": [r["elbo"]], "iters": np.asarray([r["iters"]]),   # noqa: E731
                        "labels": r["labels"], "n_clusters": np.asarray([r["n_clusters"]])}
    _assert_parity(as_run(want), want, ld, len(labels))
    with np.errstate(all="ignore"):
        mutant = _vbx_mutant(y, labels, case["phi"], *case["params"], max_iters=M.ITERS)
    return _rejects(_assert_parity, as_run(mutant), want, ld, len(labels))


def _power_adapt(case):
    """delta delta^T not subtracted from the second moment: the update with mean_diff_scale + 1"""
    import adapt_model as AM
    from test_gpu_adapt import _assert_model
    mean, T, psi = case["model"]
    rec = AM.record(case["x"], mean, case["w"])
    ws, bs, mds = case["scales"]
    return _rejects(_assert_model, AM.update_kaldi(mean, T, psi, rec, ws, bs, mds + 1.0), AM.update_kaldi(mean, T, psi, rec, ws, bs, mds))


def _power_fusion(case):
    """the Hessian term sum w s_1 dropped from the non-target class of the pass record"""
    import fusion_model as fm
    from test_gpu_fusion import _compare, _theta
    if case["form"] != "pass":
        return False
    a, c = case["a"], case["c"]
    ref = fm.pass_matrices(case["systems"], case["es"], case["ts"], a, c, _theta(case["systems"], a, c))
    _compare("the model", ref, ref)
    mutant = dict(ref, H_n=ref["H_n"].copy())
    mutant["H_n"][fm.t_index(0, 1)] = 0.0
    return _rejects(_compare, "the mutant", mutant, ref)


def _power_transform(case):
    """one weight taken with a uniform count instead of the row's (per-row counts), the last k-step dropped (a uniform count)"""
    import transform_model as M
    mean, T, psi = case["model"]
    n = case["n"] if case["form"] == "perrow" else case["uniform"]
    ref = M.model(T, mean, psi, case["x"], n)
    M.assert_well_posed(ref, case["tag"])
    M.assert_rule(M.offset_form(T, mean, psi, case["x"], n), ref, psi, n, "the NumPy evaluation")
    fault = "weight" if case["form"] == "perrow" else "kstep"
    return _rejects(M.assert_rule, M.offset_form(T, mean, psi, case["x"], n, fault=fault, n_uniform=7), ref, psi, n, fault)


def test_transform_rows_reach_the_shapes_they_name():
    """transform_rows / transform_shapes against the dispatch's own arithmetic (csrc/transform.hip: transform_plan), on three CU
    counts: every "rows" entry runs the launches it names, and together they are every block shape of both kinds of class"""
    for g in (256, 304, 64):
        for r0 in (128, 64):
            seen = set()
            for entry in sc.MENUS["transform"]["rows"]:
                r = sc.transform_rows(entry, g, r0)
                nb = -(-r // r0)
                main = min(r, nb // g * g * r0)
                tail = r - main
                per_cu = -(-tail // g)
                want = ({("main", r0)} if main else set()) | ({("tail", 16 if per_cu <= 16 else 32 if per_cu <= 32 else 64 if per_cu <= 64 else r0)} if tail else set())
                assert sc.transform_shapes(entry, r0) == want, (g, r0, entry)
                seen |= want
            assert seen == {("main", r0)} | {("tail", b) for b in ((16, 32, 64, 128) if r0 == 128 else (16, 32, 64))}


POWER = {"topn": _power_topn, "transform": _power_transform, "der": _power_der, "ahc": _power_ahc, "asnorm": _power_asnorm, "mindcf": _power_mindcf,
         "calibration": _power_calibration, "embed": _power_embed, "vbx": _power_vbx, "adapt": _power_adapt, "fusion": _power_fusion}


def test_the_ahc_mutant_differs_from_the_model_only_at_ties():
    import ahc_model as M
    from test_gpu_ahc import _assert_equal
    S = M.gaussian(40, 3)
    _assert_equal(M.cluster([S], 0.0, 2, one=_ahc_mutant_one), M.cluster([S], 0.0, 2))


@pytest.mark.parametrize("module", sc.MODULES)
def test_a_planted_mutant_of_the_model_is_rejected(module, monkeypatch):
    assert sorted(POWER) == sorted(sc.MODULES)
    fn = POWER[module]
    args = (monkeypatch,) if fn.__code__.co_argcount == 2 else ()
    caught = [c["tag"] for c in _committed(module) if fn(c, *args)]
    print("%s: the mutant is rejected on %d of %d cases" % (module, len(caught), sc.COUNTS[module]))
    assert caught, "%s: no committed case tells the mutant from the model" % module
