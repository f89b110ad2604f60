"""GPU: corpus-scale clustering (csrc/ahc.hip, the wide class; include/plda_hip.h "corpus-scale clustering", K28): ONE problem
spread over the whole device, held to the NumPy model of the speaker clustering (tests/ahc_model.py) with R = 1, and to the
one-workgroup classes at N = 4096.  The contract is exact: every comparison is array_equal on the bits, no tolerances.

Every device call goes through _run: the scores sit between NaN neighbours (and, at a row stride above N, NaN padding), every
output between guard bands filled with a payload that must stay intact outside the output and be gone inside it (the patterns
of tests/test_gpu_ahc.py)."""
import ctypes as C
import gc

import numpy as np
import pytest

import ahc_model as M
import ahc_wide_model as W

pytestmark = pytest.mark.gpu

GUARD = 16 << 10           # elements on either side
PAYLOAD = 0x7FC0DEAD
E_INVAL = -1


def _dev():
    import torch
    return torch.device("cuda", 0)


def _guarded_input(a):
    """a 1-D host array inside a device buffer whose neighbours are NaN"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(GUARD + t.numel() + GUARD, dtype=t.dtype, device=_dev())
    buf.fill_(float("nan"))
    body = buf[GUARD:GUARD + t.numel()]
    body.copy_(t.to(_dev()))
    return buf, body


class _Out:
    """a 1-D output of `count` elements between guard bands, everything pre-filled with the payload"""

    def __init__(self, count, dtype):
        import torch
        self.count = count
        self.words_per = torch.empty(0, dtype=dtype).element_size() // 4
        n = (GUARD + count + GUARD) * self.words_per
        self.words = torch.full((n,), PAYLOAD, dtype=torch.int32, device=_dev())
        self.body = self.words.view(dtype)[GUARD:GUARD + count]

    def ptr(self):
        return self.body.data_ptr() if self.count else self.words.view(self.body.dtype)[GUARD:].data_ptr()

    def check(self, what, written=True):
        w = self.words.cpu().numpy().reshape(-1, self.words_per)
        lo, hi = GUARD, GUARD + self.count
        assert (w[:lo] == np.int32(PAYLOAD)).all() and (w[hi:] == np.int32(PAYLOAD)).all(), "%s: guard band overwritten" % what
        if written:
            left = int((w[lo:hi] == np.int32(PAYLOAD)).all(1).sum())
            assert left == 0, "%s: %d output elements never written" % (what, left)
        return self.body.cpu().numpy().copy()


def _lib():
    from plda_amd import _native as N
    return N.load()


def _vp(x):
    return C.c_void_p(int(x)) if x else None


def _stop(n, threshold, num_speakers):
    from plda_amd import diarize
    return diarize.wide_args(n, threshold, num_speakers)


def _outs(n):
    import torch
    return (_Out(n, torch.int32), _Out(1, torch.int32), _Out(n - 1, torch.int32), _Out(n - 1, torch.int32), _Out(n - 1, torch.float64))


def _collect(outs, merges, expect):
    import torch
    names = ("labels", "n_clusters", "merge_a", "merge_b", "merge_cost")
    if expect:
        for o, name in zip(outs, names):
            o.check(name, written=False)
        return expect
    res = [outs[0].check("labels"), outs[1].check("n_clusters")]
    for o, name in zip(outs[2:], names[2:]):
        res.append(o.check(name) if merges else None)
        if not merges:
            o.check(name, written=False)
            assert (o.body.view(torch.int32) == PAYLOAD).all()
    return tuple(res)


def _run(eng, S, threshold=None, num_speakers=1, merges=True, ld=None, expect=0):
    """plda_ahc_wide_matrix_dev on guarded buffers -> (labels, n_clusters [1], merge_a, merge_b, merge_cost) (merges=False: the
    last three None), or the status code when expect != 0"""
    import torch
    n = S.shape[0]
    ld = n if ld is None else ld
    has_t, thr, minc = _stop(n, threshold, num_speakers)
    _, ds = _guarded_input(W.with_row_stride(np.asarray(S, np.float32), ld))
    outs = _outs(n)
    torch.cuda.synchronize()
    ptrs = [outs[0].ptr(), outs[1].ptr()] + ([o.ptr() for o in outs[2:]] if merges else [None, None, None])
    rc = _lib().plda_ahc_wide_matrix_dev(eng._h, _vp(ds.data_ptr()), n, ld, has_t, thr, minc, *[_vp(p) for p in ptrs])
    torch.cuda.synchronize()
    assert rc == expect, "status %d: %s" % (rc, eng._lib.plda_last_error(eng._h).decode())
    return _collect(outs, merges, expect)


def _run_operands(eng, dX, threshold, num_speakers):
    """plda_score_ahc_wide_dev with guarded outputs"""
    import torch
    n = dX.shape[0]
    has_t, thr, minc = _stop(n, threshold, num_speakers)
    outs = _outs(n)
    torch.cuda.synchronize()
    rc = _lib().plda_score_ahc_wide_dev(eng._h, _vp(dX.data_ptr()), n, has_t, thr, minc, *[_vp(o.ptr()) for o in outs])
    torch.cuda.synchronize()
    assert rc == 0, "status %d: %s" % (rc, eng._lib.plda_last_error(eng._h).decode())
    return _collect(outs, True, 0)


def _assert_equal(got, want, what=""):
    for g, w, name in zip(got, want, ("labels", "n_clusters", "merge_a", "merge_b", "merge_cost")):
        if g is None or w is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), "%s %s: %d of %d differ" % (what, name, int((g != w).sum()), g.size)


@pytest.fixture(scope="module")
def eng():
    from plda_amd import MPlda
    return MPlda(0)


def _engine(monkeypatch, poison=False, batch=None, pieces=None):
    from plda_amd import MPlda
    env = {"PLDA_SCRATCH_POISON": "1" if poison else None, "PLDA_AHC_WIDE_BATCH": batch, "PLDA_AHC_WIDE_PIECES": pieces}
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))
    e = MPlda(0)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    return e


FAMILIES = {"gaussian": lambda n: M.gaussian(n, 7 * n + 1), "integers": lambda n: M.integers(n, 3 * n + 2), "chain": lambda n: M.chain(n),
            "chain_reverse": lambda n: M.chain(n, True), "equal": lambda n: M.all_equal(n), "zeros": lambda n: M.signed_zeros(n, n)}
_REF = {}


def _ref(family, n):
    """the model's full merge record of one block, computed once per (family, n) and left unchanged"""
    if (family, n) not in _REF:
        S = FAMILIES[family](n)
        S.setflags(write=False)
        _REF[family, n] = (S, M.cluster([S], None, 1))
    return _REF[family, n]


def test_plan_reports_the_class(eng, monkeypatch):
    from plda_amd import diarize
    assert diarize.AHC_WIDE_MAX == 32768
    p = diarize.plan_wide(eng, 1000)
    assert p["launches_per_step"] == 3 and p["steps_per_check"] >= 1 and p["pieces"] == 1
    assert 8 * 1000 * 1000 <= p["scratch_bytes"] < 8 * 1000 * 1000 + (1 << 20)
    big = diarize.plan_wide(eng, 32768)
    assert big["scratch_bytes"] >= 8 << 30 and 1 < big["pieces"] <= 64
    knobs = _engine(monkeypatch, batch=7, pieces=3)
    assert diarize.plan_wide(knobs, 1000)["steps_per_check"] == 7 and diarize.plan_wide(knobs, 1000)["pieces"] == 3
    out = (C.c_int64 * 4)()
    assert _lib().plda_ahc_wide_plan(eng._h, 0, out) == E_INVAL and _lib().plda_ahc_wide_plan(eng._h, 32769, out) == E_INVAL
    assert "PLDA_AHC_WIDE_MAX" in eng._lib.plda_last_error(eng._h).decode()


# N on both sides of the update kernel's 256 rows per workgroup (and of a piece's length granule, also 256), and of the 128
# list rows one rescan grid takes before it strides
SIZES = {"small": [1, 2, 3, 63, 64, 65], "rows128": [127, 128, 129], "rows256": [255, 256, 257], "rows512": [511, 512, 513]}


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("which", sorted(SIZES))
def test_full_merge_record_equals_the_model(eng, family, which):
    for n in SIZES[which]:
        S, want = _ref(family, n)
        _assert_equal(_run(eng, S, None, 1), want, "%s n=%d" % (family, n))


@pytest.mark.parametrize("family", ["gaussian", "integers"])
def test_full_merge_record_at_1025(eng, family):
    S, want = _ref(family, 1025)
    _assert_equal(_run(eng, S, None, 1), want, "%s n=1025" % family)


@pytest.mark.parametrize("rule", ["above_every_score", "mid_inside_a_batch", "mid_at_a_batch_boundary", "count_1", "count_n",
                                  "both_count_binds", "both_threshold_binds"])
def test_stop_rules(monkeypatch, rule):
    """one gaussian block of 300 on a handle whose host check comes every 7 steps: 35 merges end exactly at a check, 38 inside
    a batch"""
    e = _engine(monkeypatch, batch=7)
    n = 300
    S, full = _ref("gaussian", n)
    costs = full[4]
    thr, ns = {"above_every_score": (1e6, None), "mid_inside_a_batch": (W.threshold_after(costs, 38), None),
               "mid_at_a_batch_boundary": (W.threshold_after(costs, 35), None), "count_1": (None, 1), "count_n": (None, n),
               "both_count_binds": (W.threshold_after(costs, 38), 280), "both_threshold_binds": (W.threshold_after(costs, 38), 100)}[rule]
    want = M.cluster([S], thr, ns)
    got = _run(e, S, thr, ns)
    _assert_equal(got, want, rule)
    made = int((got[2] >= 0).sum())
    assert made == {"above_every_score": 0, "mid_inside_a_batch": 38, "mid_at_a_batch_boundary": 35, "count_1": n - 1, "count_n": 0,
                    "both_count_binds": 20, "both_threshold_binds": 38}[rule]
    assert got[1].tolist() == [n - made]
    if made == 0:                                         # the whole record is tail
        assert (got[2] == -1).all() and (got[3] == -1).all() and np.isposinf(got[4]).all()
    _assert_equal(_run(e, S, thr, ns, merges=False), want[:2] + (None, None, None), rule + " without merges")


def test_result_does_not_depend_on_the_knobs_the_scratch_or_the_history(monkeypatch):
    """steps per host check in {1, 7, default} x row-scan pieces in {1, 3, default}, fresh and poisoned scratch, and a handle
    that ran a larger problem, the one-workgroup class and a smaller problem first: every output bit-identical.  513 columns in
    3 pieces of 256: the last piece holds one column; 511 and 512: it is empty."""
    from plda_amd import diarize
    cases = []
    for family, n in (("gaussian", 513), ("integers", 513), ("integers", 511), ("gaussian", 512)):
        S, full = _ref(family, n)
        cases.append((S, None, 1, full))
    S, full = _ref("gaussian", 513)
    thr = W.threshold_after(full[4], 100)
    cases.append((S, thr, 3, M.cluster([S], thr, 3)))
    for poison in (False, True):
        for batch in (1, 7, None):
            for pieces in (1, 3, None):
                if poison and (batch, pieces) not in ((7, 3), (None, None)):
                    continue
                e = _engine(monkeypatch, poison, batch, pieces)
                for i, (S, t, ns, want) in enumerate(cases):
                    _assert_equal(_run(e, S, t, ns), want, "poison %r batch %r pieces %r case %d" % (poison, batch, pieces, i))
                e.synchronize()
                del e
    e = _engine(monkeypatch, pieces=3)                     # (and the poison switch off again for whatever runs next)
    S, t, ns, want = cases[-1]
    fresh = _run(e, S, t, ns)
    big, big_want = _ref("integers", 1025)
    _assert_equal(_run(e, big, None, 1), big_want, "the larger problem")
    diarize.ahc(e, [M.gaussian(300, 4), M.gaussian(40, 5)], 0.0)
    _assert_equal(_run(e, M.gaussian(70, 1), None, 1), M.cluster([M.gaussian(70, 1)], None, 1), "the smaller problem")
    _assert_equal(_run(e, S, t, ns), fresh, "after other calls")
    _assert_equal(fresh, want, "fresh")


@pytest.mark.parametrize("family", ["gaussian", "integers"])
def test_wide_class_equals_the_one_workgroup_class_at_4096(eng, family):
    """the same block through plda_ahc_wide_matrix_dev (ld = N and ld = N + 5) and plda_ahc_matrix_dev: the full merge records
    are equal"""
    import torch
    from plda_amd import diarize
    n = 4096
    S = FAMILIES[family](n)
    wide = _run(eng, S, None, 1)
    _assert_equal(_run(eng, S, None, 1, ld=n + 5), wide, "ld = N + 5")
    scores, block_off, offsets = diarize.pack([S])
    _, ds = _guarded_input(scores)
    outs = _outs(n)
    torch.cuda.synchronize()
    eng.ahc_matrix_dev(ds.data_ptr(), block_off, offsets, 0, 0.0, np.ones(1, np.int32), *[o.ptr() for o in outs])
    torch.cuda.synchronize()
    _assert_equal(wide, _collect(outs, True, 0), "wide against the HBM class")
    assert (wide[2] >= 0).all() and wide[1].tolist() == [1]


def _unequal_sizes(total, groups, seed):
    rng = np.random.default_rng(seed)
    w = rng.random(groups) + 0.2
    s = np.maximum(1, np.floor(w / w.sum() * total).astype(np.int64))
    s[0] += total - s.sum()
    assert s.sum() == total and s.min() >= 1 and len(set(s.tolist())) > groups // 2
    return s


def test_planted_groups_at_256_equal_the_model(eng):
    S, g = M.planted(_unequal_sizes(256, 16, 9), seed=9)
    want = M.cluster([S], 0.0, None)
    assert np.array_equal(want[0], M.first_member_labels(g)) and want[1].tolist() == [16]
    _assert_equal(_run(eng, S, 0.0, None), want, "n = 256")


@pytest.mark.parametrize("n", [4097, 8192])
def test_above_the_old_limit(eng, n):
    """N above PLDA_AHC_MAX: 16 planted groups of unequal sizes, +1 inside and -1 across, threshold 0 (every within-group pair
    ties at every step).  Only the labels are checked: the groups numbered by first member; that the RULE yields this answer is
    shown by the model on the same construction at N = 256 (the test above)."""
    S, g = M.planted(_unequal_sizes(n, 16, n), seed=n)
    labels, ncl, _, _, _ = _run(eng, S, 0.0, None, merges=False)
    assert ncl.tolist() == [16]
    assert np.array_equal(labels, M.first_member_labels(g))


# ------------------------------------------------------------------------------------------- operand form, host forms
def _model_params(d, seed, psi_scale=1.0):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    return rng.random(d), q * (0.5 + rng.random(d))[:, None], np.sort(rng.random(d) * 3.0 + 0.05)[::-1].copy() * psi_scale


def _speaker_rows(n, d, seed):
    rng = np.random.default_rng(seed)
    spk = rng.standard_normal((6, d)) * 1.5
    return spk[rng.integers(0, 6, n)] + rng.standard_normal((n, d))


def _scored_block(e, dX):
    """the block plda_score_matrix_dev writes from the device rows dX (ld_out = N)"""
    import torch
    n = dX.shape[0]
    S = torch.full((n, n), float("nan"), dtype=torch.float32, device=_dev())
    torch.cuda.synchronize()
    e.score_matrix_dev(dX.data_ptr(), None, 1, n, dX.data_ptr(), n, S.data_ptr(), n)
    e.synchronize()
    return S.cpu().numpy()


@pytest.mark.parametrize("d", [8, 200])
@pytest.mark.parametrize("n", [130, 1025])
def test_operand_form_equals_matrix_form_on_the_scored_block(eng, d, n):
    import torch
    from plda_amd import diarize
    eng.set_model(*_model_params(d, d))
    vecs = _speaker_rows(n, d, d + n)
    dX = torch.from_numpy(vecs).to(_dev())
    S = _scored_block(eng, dX)
    for thr, ns in ((None, 1), (0.0, None), (5.0, 3)):
        got = _run_operands(eng, dX, thr, ns)
        _assert_equal(got, _run(eng, S, thr, ns), "operand against matrix form")
        if n == 130:
            _assert_equal(got, M.cluster([S], thr, ns), "operand form against the model")
            labels, k, mg = diarize.ahc_wide_vectors(eng, vecs, thr, ns, return_merges=True)
            _assert_equal((labels, np.asarray([k], np.int32)) + mg, got, "host operand form")


def test_operand_form_on_a_cosine_handle():
    import torch
    from plda_amd import Cosine
    c = Cosine(8)
    vecs = _speaker_rows(130, 8, 99)
    dX = torch.from_numpy(vecs).to(_dev())
    S = _scored_block(c, dX)
    assert np.abs(S).max() <= 1.0 + 1e-6                                  # cosines
    got = _run_operands(c, dX, 0.3, None)
    _assert_equal(got, _run(c, S, 0.3, None), "cosine operand against matrix form")
    _assert_equal(got, M.cluster([S], 0.3, None), "cosine operand form against the model")
    labels, k = c.cluster_corpus(vecs, threshold=0.3)
    _assert_equal((labels, np.asarray([k], np.int32)), got[:2], "Cosine.cluster_corpus")


def test_host_form_equals_device_form(eng):
    from plda_amd import diarize
    S, _ = _ref("integers", 257)
    for thr, ns in ((None, 1), (0.0, 2)):
        want = _run(eng, S, thr, ns)
        labels, k, mg = diarize.ahc_wide(eng, S, thr, ns, return_merges=True)
        _assert_equal((labels, np.asarray([k], np.int32)) + mg, want, "host form")
        labels, k = diarize.ahc_wide(eng, S, thr, ns)
        _assert_equal((labels, np.asarray([k], np.int32)), want[:2], "host form without merges")
    labels, k = diarize.ahc_wide(eng, np.zeros((1, 1), np.float32), 0.0)
    assert labels.tolist() == [0] and k == 1


def test_non_finite_scores_fail_with_the_count(eng):
    S = M.gaussian(300, 2).copy()
    S[7, 7] = np.inf                                       # the diagonal is never read
    _assert_equal(_run(eng, S, 0.0, None), M.cluster([S], 0.0, None), "inf on the diagonal")
    S[1, 4] = np.nan
    S[200, 3] = -np.inf
    S[299, 0] = np.inf
    assert _run(eng, S, 0.0, None, expect=E_INVAL) == E_INVAL
    assert "3 non-finite" in eng._lib.plda_last_error(eng._h).decode()
    assert _run(eng, S, None, 1, ld=305, expect=E_INVAL) == E_INVAL       # (the NaN padding of the rows is not counted)
    assert "3 non-finite" in eng._lib.plda_last_error(eng._h).decode()
    clean = S[100:120, 100:120].copy()                     # (none of the four lies in it)
    _assert_equal(_run(eng, clean, 0.0, None), M.cluster([clean], 0.0, None), "after a failure")


def test_bad_arguments(eng):
    import torch
    n = 4
    ds = torch.from_numpy(M.gaussian(n, 1).ravel()).to(_dev())
    L, K = torch.zeros(n, dtype=torch.int32, device=_dev()), torch.zeros(1, dtype=torch.int32, device=_dev())
    A, B = torch.zeros(n - 1, dtype=torch.int32, device=_dev()), torch.zeros(n - 1, dtype=torch.int32, device=_dev())
    Cc = torch.zeros(n - 1, dtype=torch.float64, device=_dev())
    full = [L.data_ptr(), K.data_ptr(), A.data_ptr(), B.data_ptr(), Cc.data_ptr()]
    err = lambda: eng._lib.plda_last_error(eng._h).decode()      # noqa: E731

    def call(N=n, ld=n, has_t=1, thr=0.0, minc=1, outs=full, scores=ds.data_ptr()):
        return _lib().plda_ahc_wide_matrix_dev(eng._h, _vp(scores), N, ld, has_t, thr, minc, *[_vp(o) for o in outs])

    assert call() == 0
    for bad_n in (0, -1, 32769):
        assert call(N=bad_n, ld=max(bad_n, 1)) == E_INVAL and "N = " in err() and "PLDA_AHC_WIDE_MAX" in err()
    assert call(ld=n - 1) == E_INVAL and "ld = 3" in err()
    assert call(thr=float("nan")) == E_INVAL and "threshold is NaN" in err()
    assert call(has_t=0, thr=float("nan")) == 0                           # (no threshold: the value is not looked at)
    for bad in (0, -3):
        assert call(minc=bad) == E_INVAL and "min_clusters = %d" % bad in err()
    assert call(scores=None) == E_INVAL and "scores" in err()
    assert call(outs=[None] + full[1:]) == E_INVAL and "labels" in err()
    assert call(outs=[full[0], None] + full[2:]) == E_INVAL and "n_clusters" in err()
    for keep in range(3):                                                 # one merge pointer alone, or two
        assert call(outs=full[:2] + [full[2 + j] if j == keep else None for j in range(3)]) == E_INVAL and "together" in err()
        assert call(outs=full[:2] + [None if j == keep else full[2 + j] for j in range(3)]) == E_INVAL and "together" in err()
    assert call(outs=full[:2] + [None, None, None]) == 0
    eng.set_model(*_model_params(4, 1))
    dX = torch.zeros((n, 4), dtype=torch.float64, device=_dev())
    op = lambda N=n, minc=1, x=dX.data_ptr(): _lib().plda_score_ahc_wide_dev(eng._h, _vp(x), N, 1, 0.0, minc, *[_vp(o) for o in full])  # noqa: E731
    assert op(N=0) == E_INVAL and op(N=32769) == E_INVAL and "PLDA_AHC_WIDE_MAX" in err()
    assert op(minc=0) == E_INVAL and "min_clusters" in err()
    assert op(x=None) == E_INVAL and "X is NULL" in err()


def test_create_cluster_destroy_gives_back_every_byte():
    from plda_amd import MPlda, diarize
    S = M.gaussian(300, 2)
    vecs = np.random.default_rng(6).standard_normal((80, 16))
    gc.collect()
    first = _lib().plda_device_bytes_held()
    for cycle in range(10):
        e = MPlda(0)
        diarize.ahc_wide(e, S, 0.0)
        e.set_model(*_model_params(16, 2))
        diarize.ahc_wide_vectors(e, vecs, 0.0)
        assert _lib().plda_device_bytes_held() >= first + 8 * 300 * 300
        del e
        gc.collect()
        held = _lib().plda_device_bytes_held()
        assert held == first, "cycle %d: %d bytes of device memory not given back" % (cycle, held - first)


# ------------------------------------------------------------------------------------------- clustering-based adaptation
def _generate(mean, T, psi, counts, rng):
    """rows from the model's own generative form: u = y_speaker + e in the model's space (y ~ N(0, psi), e ~ N(0, I)),
    x = mean + T^-1 u; the speakers' rows interleaved at random -> (rows, speaker of each row)"""
    d = len(mean)
    g = rng.permutation(np.repeat(np.arange(len(counts)), counts))
    y = rng.standard_normal((len(counts), d)) * np.sqrt(psi)
    u = y[g] + rng.standard_normal((len(g), d))
    return mean + u @ np.linalg.inv(T).T, g


def test_adapt_clustered_equals_the_steps_done_by_hand():
    """300 rows of 10 well-separated speakers of a known model (between-speaker variances 400 x those of _model_params) and 3
    singleton outliers: the labels recover the planted partition, min_cluster_size = 2 drops the outliers, and the adapted
    model is bit-equal to cluster_corpus -> filter (the host model) -> MPlda.fit on a second handle -> blend"""
    from liblda.plda import PLDA
    from plda_amd import MPlda
    d, counts = 8, (30,) * 10 + (1, 1, 1)
    mean, T, psi = _model_params(d, 31, psi_scale=400.0)
    rng = np.random.default_rng(31)
    x, g = _generate(mean, T, psi, counts, rng)
    x = x + 0.25                                          # the in-domain data is shifted
    p = PLDA(0)
    p._instance.set_model(mean, T, psi)
    p._instance._meanz[3] = 1.0
    rec = p.adapt_clustered(x, threshold=None, num_speakers=13, alpha=0.3, min_cluster_size=2, iters=5)
    assert np.array_equal(rec.labels, M.first_member_labels(g)) and rec.labels.dtype == np.int32
    assert (rec.n_clusters, rec.rows_kept, rec.clusters_kept) == (13, 300, 10)
    assert p._instance._meanz == {} and p._instance._calibration is None
    b = MPlda(0)
    b.set_model(mean, T, psi)
    labels, ncl = b.cluster_corpus(x, threshold=None, num_speakers=13)
    assert np.array_equal(labels, rec.labels) and ncl == 13
    rows, new_labels, kept = W.keep_clusters(labels, 2)
    assert kept == 10 and len(rows) == 300 and np.array_equal(np.sort(g[rows]), np.repeat(np.arange(10), 30))
    c = MPlda(0)
    c.fit(np.ascontiguousarray(x[rows]), new_labels.astype(np.uint64), 5)
    b.blend(c, 0.3)
    got, want = p._instance.get_model(), b.get_model()
    for k in ("mean", "transform", "psi"):
        assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), k
    assert not np.array_equal(got["mean"], mean)
    with pytest.raises(ValueError, match="an in-domain model needs two"):
        b.adapt_clustered(x, threshold=None, num_speakers=13, min_cluster_size=31)
    after = b.get_model()
    assert all(np.array_equal(after[k], want[k]) for k in ("mean", "transform", "psi"))      # (the model untouched)
