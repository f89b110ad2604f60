"""GPU: trial keys (csrc/partition.hip; include/plda_hip.h "trial keys") against the NumPy statement tests/trialkey_model.py.
Lists are compared as uint32 views with np.array_equal, counts with ==.  Shapes are the smallest at which the kernel can go
wrong: partial last strips and widths not divisible by four, the four-row unroll's tail, the vector and the two scalar
layouts, slices of 3 and 64 rows beside the planner's; keys from "everything" to sixteen lists in one row-strip, a row-strip
all of one list (the 8-bit wrap) and nothing at all.  Then the order contract, score bits, guards, poisoned scratch, a
long-lived handle, the operand form, the device-list consumers against their host siblings, rule="all" against the matrix
forms, and PLDA.evaluate on a fitted model."""
import ctypes as C
import os

import numpy as np
import pytest

import trialkey_model as TM

pytestmark = pytest.mark.gpu

ENV = ("PLDA_EER_SLAB_ROWS", "PLDA_SCRATCH_POISON", "PLDA_PARTITION_SLICE_ROWS", "PLDA_ROCCH_VARIANT", "PLDA_MINDCF_VARIANT", "PLDA_EER_VARIANT")
GUARD = 64                      # sentinel words behind each buffer's total
SENTINEL = 0x5A5A5A5A
NTS = (1, 3, 255, 256, 257, 1027)
MS = (1, 2, 5, 67)
LAYOUTS = ("vector", "pitch+3", "offset1")
KINDS = ("everything", "sixteen", "wrap_lo", "wrap_hi", "random", "nothing", "codes128")


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _make(slice_rows=0, d=0, slab=None, poison=False):
    """a fresh handle made with the suite's creation-time switches cleared around it, but these"""
    from plda_amd import MPlda
    saved = {k: os.environ.pop(k, None) for k in ENV}
    try:
        if slice_rows:
            os.environ["PLDA_PARTITION_SLICE_ROWS"] = str(slice_rows)
        if slab:
            os.environ["PLDA_EER_SLAB_ROWS"] = str(slab)
        if poison:
            os.environ["PLDA_SCRATCH_POISON"] = "1"
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
    """the planner's slice height, slices of 3 rows (the unroll's tail in every slice) and of 64"""
    return {s: _make(s) for s in (0, 3, 64)}


# ---------------------------------------------------------------------------------------------- keys and scores
def _key(kind, m, nt, rng):
    """(enrol_code, test_code, table, n_buckets, enrol_spk, test_spk)"""
    espk, tspk = rng.integers(0, 5, m).astype(np.int64), rng.integers(0, 5, nt).astype(np.int64)
    if kind == "everything":
        return np.zeros(m, np.uint8), np.zeros(nt, np.uint8), np.zeros((1, 1), np.int8), 1, espk, tspk
    if kind == "sixteen":       # column j is of bucket j % 8, speakers 0 / 1: from 16 columns on every row-strip holds all 16 lists
        tcode = (np.arange(nt) % 8).astype(np.uint8)
        return (np.zeros(m, np.uint8), tcode, np.arange(8, dtype=np.int8).reshape(1, 8), 8, rng.integers(0, 2, m).astype(np.int64),
                ((np.arange(nt) // 8) % 2).astype(np.int64))
    if kind in ("wrap_lo", "wrap_hi"):
        # even rows: every trial of a row-strip in ONE list (256 of them from Nt = 256 on) -- list 0, whose field's carry would run
        # into list 1's, or list 15, whose carry leaves the word; odd rows: the other lists mixed in
        nb, full = (2, 0) if kind == "wrap_lo" else (8, 7)
        ecode = (np.arange(m) % 2).astype(np.uint8)
        tcode = rng.integers(0, 4, nt).astype(np.uint8)
        table = np.empty((2, 4), np.int8)
        table[0], table[1] = full, rng.integers(-1, nb, 4)
        tspk[:] = 3
        espk = np.where(np.arange(m) % 2 == 0, 9 if kind == "wrap_lo" else 3, rng.integers(2, 5, m)).astype(np.int64)
        return ecode, tcode, table, nb, espk, tspk
    if kind == "nothing":
        return rng.integers(0, 3, m).astype(np.uint8), rng.integers(0, 2, nt).astype(np.uint8), np.full((3, 2), -1, np.int8), 3, espk, tspk
    ce = ct = 128 if kind == "codes128" else 6
    nb = 5
    table = rng.integers(0, nb, (ce, ct)).astype(np.int8)
    table[table == 2] = -1                      # bucket 2 is empty
    table[rng.random((ce, ct)) < 0.3] = -1
    table[1] = -1                               # a row code with no trial
    table[:, 0] = np.where(table[:, 0] >= 0, 4, -1)
    table[table == 4] = -1
    table[0, 0] = 4                             # bucket 4: test code 0 only, whose speakers no enrol row has: no target
    ecode, tcode = rng.integers(0, ce, m).astype(np.uint8), rng.integers(0, ct, nt).astype(np.uint8)
    ecode[0] = 0
    tspk[tcode == 0] = 77
    return ecode, tcode, table, nb, espk, tspk


def _scores(m, nt, rng):
    """random BIT patterns (NaNs of every payload, infinities, denormals among them) and the named specials up front"""
    S = rng.integers(0, 2 ** 32, (m, nt), dtype=np.uint64).astype(np.uint32).view(np.float32).copy()
    special = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc00001, 0xffc12345, 0x7f800001, 0x00000000], np.uint32).view(np.float32)
    flat = S.reshape(-1)
    flat[:min(len(special), flat.shape[0])] = special[:flat.shape[0]]
    return S


def _laid_out(S, layout):
    """(host buffer, offset in floats, ld): the matrix in a NaN-filled buffer"""
    m, nt = S.shape
    ld, off = {"vector": ((nt + 3) // 4 * 4, 0), "pitch+3": (nt + 3, 0), "offset1": ((nt + 3) // 4 * 4, 1)}[layout]
    buf = np.full(off + m * ld, np.nan, np.float32)
    buf[off:].reshape(m, ld)[:, :nt] = S
    return buf, off, ld


class _Run(object):
    """one raw call of plda_partition_matrix_dev / plda_score_partition_dev with sentinels behind each buffer's total"""

    def __init__(self, eng, key6, matrix=None, operands=None, cap_extra=GUARD):
        import torch
        from plda_amd import trialkey as TK
        ecode, tcode, table, nb, espk, tspk = key6
        self.key = TK.TrialKey.from_codes(ecode, tcode, table, list(range(nb)))
        self.keep = [_t(ecode), _t(tcode), _t(espk), _t(tspk)]
        want = self.key.plan(espk, tspk)[0]
        nt1, nt0 = int(want["total"][1]), int(want["total"][0])
        self.dtar = torch.full((nt1 + GUARD,), SENTINEL, dtype=torch.int32, device=_dev())
        self.dnon = torch.full((nt0 + GUARD,), SENTINEL, dtype=torch.int32, device=_dev())
        ks = self.key._struct(self.keep[0].data_ptr(), self.keep[1].data_ptr())
        self.rec = np.zeros(1, TK.RECORD_DTYPE)
        tail = [C.c_void_p(self.keep[2].data_ptr()), C.c_void_p(self.keep[3].data_ptr()), C.cast(C.byref(ks), C.c_void_p),
                C.c_void_p(self.dtar.data_ptr()), nt1 + cap_extra, C.c_void_p(self.dnon.data_ptr()), nt0 + cap_extra,
                C.c_void_p(self.rec.ctypes.data)]
        torch.cuda.synchronize()
        if matrix is not None:
            ptr, ld, m, nt = matrix
            self.rc = eng._lib.plda_partition_matrix_dev(eng._h, C.c_void_p(ptr), ld, m, nt, *tail)
        else:
            self.rc = eng._lib.plda_score_partition_dev(eng._h, *(list(operands) + tail))
        eng.synchronize()
        self.want, self.nt1, self.nt0 = want, nt1, nt0
        self.tar, self.non = self.dtar.cpu().numpy().view(np.uint32), self.dnon.cpu().numpy().view(np.uint32)

    def check(self, model, what):
        """counts ==, lists bit for bit, guards untouched"""
        from plda_amd import _native as N
        assert self.rc == N.PLDA_OK, (what, self.rc)
        count, offset, total = model["plan"]
        r = self.rec[0]
        assert np.array_equal(r["count"], count) and np.array_equal(r["offset"], offset) and np.array_equal(r["total"], total), what
        assert np.array_equal(self.tar[:self.nt1], TM.bits(model["tar"])), what
        assert np.array_equal(self.non[:self.nt0], TM.bits(model["non"])), what
        assert (self.tar[self.nt1:] == SENTINEL).all() and (self.non[self.nt0:] == SENTINEL).all(), what


def _model(S, key6):
    ecode, tcode, table, nb, espk, tspk = key6
    per, tar, non = TM.lists(S, ecode, tcode, table, nb, espk, tspk)
    return {"plan": TM.plan(ecode, tcode, table, nb, espk, tspk), "tar": tar, "non": non, "per": per}


def _matrix_run(eng, S, layout, key6, **kw):
    buf, off, ld = _laid_out(S, layout)
    d = _t(buf)
    run = _Run(eng, key6, matrix=(d.data_ptr() + 4 * off, ld, S.shape[0], S.shape[1]), **kw)
    del d
    return run


# ---------------------------------------------------------------------------------------------- the lists, at every edge
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("nt", NTS)
def test_lists_equal_the_model(engines, nt, layout):
    rng = np.random.default_rng(1000 + nt)
    seen = set()
    for m in MS:
        S = _scores(m, nt, rng)
        for kind in KINDS:
            key6 = _key(kind, m, nt, rng)
            model = _model(S, key6)
            for s, eng in engines.items():
                if s and kind not in ("sixteen", "random", "wrap_hi"):
                    continue
                _matrix_run(eng, S, layout, key6).check(model, (m, nt, layout, kind, s))
            count = model["plan"][0]
            seen.add((kind, int(np.count_nonzero(count))))
            if kind == "nothing":
                assert not count.any()
            if kind == "sixteen" and nt >= 255 and m >= 5:
                assert np.count_nonzero(count) == 16
            if kind == "random" and nt >= 255 and m == 67:
                assert count[2].sum() == 0 and count[4][1] == 0 and count[4][0] > 0 and count[0].min() > 0
    assert len(seen) >= len(KINDS)


def test_the_wrap_case_is_met():
    """the keys named wrap_* really put 256 trials of one list into one row-strip"""
    rng = np.random.default_rng(5)
    for kind, lst in (("wrap_lo", 0), ("wrap_hi", 15)):
        ecode, tcode, table, nb, espk, tspk = _key(kind, 5, 257, rng)
        bucket, cls = TM.bucket_and_class(ecode, tcode, table, espk, tspk)
        L = np.where(bucket >= 0, 2 * bucket + cls, -1)
        assert (L[0, :256] == lst).all() and (L[2, :256] == lst).all()


def test_order_is_the_keys_not_the_scores(engines):
    """two different matrices under one key: element k of every list is the same trial (the second matrix encodes i * Nt + j)"""
    rng = np.random.default_rng(11)
    m, nt = 67, 1027
    key6 = _key("random", m, nt, rng)
    S = rng.standard_normal((m, nt)).astype(np.float32)
    index = (np.arange(m)[:, None] * nt + np.arange(nt)[None, :]).astype(np.float32)          # (< 2^24: exact)
    a, b = _matrix_run(engines[0], S, "vector", key6), _matrix_run(engines[64], index, "pitch+3", key6)
    a.check(_model(S, key6), "scores")
    b.check(_model(index, key6), "indices")
    for x, y, n in ((a.tar, b.tar, a.nt1), (a.non, b.non, a.nt0)):
        at = y[:n].view(np.float32).astype(np.int64)
        assert np.array_equal(x[:n], TM.bits(S.reshape(-1)[at]))
    # within a list: by (strip, row, column)
    ecode, tcode, table, nb, espk, tspk = key6
    off, cnt = a.rec[0]["offset"], a.rec[0]["count"]
    for bkt in range(nb):
        at = b.non[off[bkt][0]:off[bkt][0] + cnt[bkt][0]].view(np.float32).astype(np.int64)
        order = np.stack([(at % nt) // 256, at // nt, at % nt], 1)
        assert (np.lexsort(order.T[::-1]) == np.arange(len(at))).all()


def test_refusals_write_nothing(engines):
    from plda_amd import _native as N
    eng = engines[0]
    rng = np.random.default_rng(13)
    m, nt = 5, 257
    S = _scores(m, nt, rng)
    good = _key("random", m, nt, rng)

    def refused(key6, text, **kw):
        run = _matrix_run(eng, S, "vector", key6, **kw)
        assert run.rc == N.PLDA_E_INVAL and text in N.last_error(eng._h), (text, run.rc, N.last_error(eng._h))
        assert (run.tar == SENTINEL).all() and (run.non == SENTINEL).all(), text

    refused(good, "the buffers hold", cap_extra=-1)
    ecode, tcode, table, nb, espk, tspk = good
    bad = ecode.copy()
    bad[4] = 200
    # (the host plan of _Run refuses a bad key first: build the run around a good plan, then swap the device codes)
    import torch
    from plda_amd import trialkey as TK
    key = TK.TrialKey.from_codes(ecode, tcode, table, list(range(nb)))
    dS, des, dts, dbad, dtc = _t(S), _t(espk), _t(tspk), _t(bad), _t(tcode)
    dtar = torch.full((m * nt,), SENTINEL, dtype=torch.int32, device=_dev())
    dnon = torch.full((m * nt,), SENTINEL, dtype=torch.int32, device=_dev())
    rec = np.zeros(1, TK.RECORD_DTYPE)

    def call(ks, ld=nt, mm=m):
        torch.cuda.synchronize()
        return eng._lib.plda_partition_matrix_dev(eng._h, C.c_void_p(dS.data_ptr()), ld, mm, nt, C.c_void_p(des.data_ptr()),
                                                  C.c_void_p(dts.data_ptr()), C.cast(C.byref(ks), C.c_void_p) if ks is not None else None,
                                                  C.c_void_p(dtar.data_ptr()), m * nt, C.c_void_p(dnon.data_ptr()), m * nt,
                                                  C.c_void_p(rec.ctypes.data))

    for ks, kw, text in ((key._struct(dbad.data_ptr(), dtc.data_ptr()), {}, "enrol_code[4]"),
                         (None, {}, "NULL"),
                         (key._struct(None, dtc.data_ptr()), {}, "NULL"),
                         (key._struct(dbad.data_ptr(), dtc.data_ptr()), {"ld": nt - 1}, "bad argument"),
                         (key._struct(dbad.data_ptr(), dtc.data_ptr()), {"mm": 0}, "bad argument")):
        assert call(ks, **kw) == N.PLDA_E_INVAL and text in N.last_error(eng._h), (text, N.last_error(eng._h))
    nine = TK._Key(dbad.data_ptr(), dtc.data_ptr(), table.ctypes.data, table.shape[0], table.shape[1], 9, 0)
    assert call(nine) == N.PLDA_E_INVAL and "buckets" in N.last_error(eng._h)
    eng.synchronize()
    assert (dtar.cpu().numpy().view(np.uint32) == SENTINEL).all() and (dnon.cpu().numpy().view(np.uint32) == SENTINEL).all()
    # the device-list forms refuse what their host siblings refuse, in their words
    out = np.zeros(6)
    pos = np.zeros(3, np.float32)
    for fn, args in ((eng._lib.plda_eer_lists, (C.c_void_p(pos.ctypes.data), 0, C.c_void_p(pos.ctypes.data), 3)),
                     (eng._lib.plda_eer_lists_dev, (C.c_void_p(dS.data_ptr()), 0, C.c_void_p(dS.data_ptr()), 3))):
        assert fn(eng._h, *(args + (C.c_void_p(out.ctypes.data),))) == N.PLDA_E_INVAL
        assert N.last_error(eng._h) == "eer: need at least one target and one impostor score"


# ---------------------------------------------------------------------------------------------- poison, history
def _cases(eng, also=None):
    rng = np.random.default_rng(17)
    out = {}
    for m, nt, kind in ((67, 1027, "random"), (5, 257, "sixteen"), (67, 255, "wrap_hi")):
        S = _scores(m, nt, rng)
        key6 = _key(kind, m, nt, rng)
        if also is not None:
            also(eng)
        run = _matrix_run(eng, S, "pitch+3", key6)
        run.check(_model(S, key6), (m, nt, kind))
        out["tar_%d_%d" % (m, nt)], out["non_%d_%d" % (m, nt)], out["rec_%d_%d" % (m, nt)] = run.tar, run.non, run.rec
    return out


def _unrelated(eng):
    from plda_amd import dcf as DC
    from plda_amd import eer as EE
    rng = np.random.default_rng(19)
    m, nt = 300, 900
    es, ts = rng.integers(0, 4, m), rng.integers(0, 4, nt)
    dS, des, dts = _t(rng.standard_normal((m, nt)).astype(np.float32)), _t(es.astype(np.int64)), _t(ts.astype(np.int64))
    EE.eer_from_matrix_dev(eng, dS.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr())
    DC.min_dcf_from_matrix_dev(eng, dS.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr())


def _same_bits(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), (what, k)


def test_poisoned_scratch_two_runs_and_a_long_lived_handle():
    """under PLDA_SCRATCH_POISON=1 (every allocation of the library filled with 0xFF bytes) with guard words behind each
    buffer's total; twice; and after unrelated calls on the same handle: identical bytes"""
    eng = _make(poison=True)
    first = _cases(eng)
    _same_bits(_cases(eng), first, "the same handle again")
    _same_bits(_cases(eng, also=_unrelated), first, "after unrelated calls")
    eng.synchronize()
    del eng
    plain = _make()                            # the poison switch off again for whatever runs next in this process
    _same_bits(_cases(plain), first, "a fresh handle without poison")


# ---------------------------------------------------------------------------------------------- the operand form
def _operands(rng, m, nt, d, mixed=True, zn=True):
    spk = rng.standard_normal((12, d)) * 1.5
    es, ts = rng.integers(0, 12, m), rng.integers(0, 12, nt)
    U, V = spk[es] + rng.standard_normal((m, d)), spk[ts] + rng.standard_normal((nt, d))
    n = rng.integers(1, 4, m).astype(np.int32)
    dzm, dzs = (_t(rng.standard_normal(m)), _t(0.5 + rng.random(m))) if zn else (None, None)
    return _t(U), _t(V), (_t(n) if mixed else None), (0 if mixed else 2), dzm, dzs, es.astype(np.int64), ts.astype(np.int64)


@pytest.mark.parametrize("slice_rows", [0, 100])
def test_operand_form_is_score_matrix_plus_partition(slice_rows):
    """PLDA_EER_SLAB_ROWS=256 and M = 515: three slabs, the last of three rows; slices of 100 rows are cut by the slab boundaries"""
    import torch
    d, m, nt = 48, 515, 1027
    eng = _make(slice_rows, d=d, slab=256)
    rng = np.random.default_rng(23)
    dU, dV, dn, nu, dzm, dzs, es, ts = _operands(rng, m, nt, d)
    key6 = _key("random", m, nt, rng)[:4] + (es, ts)
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    S = torch.empty((m, nt), dtype=torch.float32, device=_dev())
    torch.cuda.synchronize()
    eng.score_matrix_dev(dU.data_ptr(), ptr(dn), nu, m, dV.data_ptr(), nt, S.data_ptr(), nt, ptr(dzm), ptr(dzs))
    eng.synchronize()
    mat = _Run(eng, key6, matrix=(S.data_ptr(), nt, m, nt))
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    opr = _Run(eng, key6, operands=[p(dU), p(dn), nu, m, p(dV), nt, p(dzm), p(dzs)])
    model = _model(S.cpu().numpy(), key6)
    mat.check(model, "matrix form")
    opr.check(model, "operand form")
    assert np.array_equal(opr.tar, mat.tar) and np.array_equal(opr.non, mat.non)
    assert model["plan"][2].min() > 1000


# ---------------------------------------------------------------------------------------------- the consumers on device lists
def _finite_case(rng, m, nt, kind="random"):
    key6 = _key(kind, m, nt, rng)
    ecode, tcode, table, nb, espk, tspk = key6
    S = (rng.standard_normal((m, nt)) + 2.0 * (espk[:, None] == tspk[None, :])).astype(np.float32)
    return S, key6


def _partition_of(eng, S, key6, names=None):
    from plda_amd import trialkey as TK
    ecode, tcode, table, nb, espk, tspk = key6
    key = TK.TrialKey.from_codes(ecode, tcode, table, names or list(range(nb)))
    return TK.partition_matrix_dev(eng, key, _t(S), _t(espk), _t(tspk))


def _same_fields(a, b, what):
    """two result objects (or dicts) field by field: floats and arrays by their bits (NaN equals NaN), the rest with =="""
    a, b = (a if isinstance(a, dict) else a.__dict__), (b if isinstance(b, dict) else b.__dict__)
    assert sorted(a) == sorted(b), what
    for k, v in a.items():
        if isinstance(v, (float, np.floating, np.ndarray)):
            u, w = np.ascontiguousarray(v), np.ascontiguousarray(b[k])
            assert u.dtype == w.dtype and u.shape == w.shape and u.tobytes() == w.tobytes(), (what, k)
        else:
            assert v == b[k], (what, k)


def test_device_list_consumers_equal_their_host_siblings(engines):
    from plda_amd import calibration as CB
    from plda_amd import dcf as DC
    from plda_amd import eer as EE
    from plda_amd import fusion as FU
    from plda_amd import rocch as RC
    from plda_amd import trialkey as TK
    eng = engines[0]
    rng = np.random.default_rng(29)
    m, nt = 67, 1027
    S, key6 = _finite_case(rng, m, nt)
    S2 = (S * 0.5 + rng.standard_normal((m, nt)) * 0.7).astype(np.float32)
    part, part2 = _partition_of(eng, S, key6), _partition_of(eng, S2, key6)
    model, model2 = _model(S, key6), _model(S2, key6)
    nb = key6[3]
    assert np.array_equal(part.counts, model["plan"][0][:nb])
    points = ((0.01, 1.0, 1.0), (0.05, 1.0, 10.0))
    cases = [(part.tar(b), part.non(b), part2.tar(b), part2.non(b), model["per"][(b, 1)], model["per"][(b, 0)], model2["per"][(b, 1)],
              model2["per"][(b, 0)], "bucket %d" % b) for b in range(nb) if min(part.counts[b]) > 0]
    cases.append(part.pooled() + part2.pooled() + (model["tar"], model["non"], model2["tar"], model2["non"], "pooled"))
    assert len(cases) == 4          # buckets 0, 1, 3 and the pool: 2 is empty, 4 has no target
    for dt, dn_, dt2, dn2, ht, hn, ht2, hn2, what in cases:
        assert np.array_equal(dt.cpu().numpy().view(np.uint32), TM.bits(ht)) and np.array_equal(dn_.cpu().numpy().view(np.uint32), TM.bits(hn))
        # the EER's six numbers
        assert np.array_equal(TK.eer_lists_dev(eng, dt, dn_)[:4], np.array(EE.eer_from_lists(eng, ht, hn))), what
        assert tuple(TK.eer_lists_dev(eng, dt, dn_)[4:]) == (len(ht), len(hn))
        for a, b in zip(TK.det_lists_dev(eng, dt, dn_, 50), EE.det_from_lists(eng, ht, hn, 50)):
            assert np.array_equal(a, b), what
        assert TK.min_dcf_lists_dev(eng, dt, dn_, points)[0] == DC.min_dcf_from_lists(eng, ht, hn, points)[0], what
        for a, c, th in ((1.0, 0.0, 0.0), (0.7, -0.3, 0.4)):
            _same_fields(TK.calib_pass_lists_dev(eng, dt, dn_, a, c, th), CB.pass_from_lists(eng, ht, hn, a, c, th), what)
        _same_fields(TK.calib_fit_lists_dev(eng, dt, dn_, 0.3), CB.fit_from_lists(eng, ht, hn, 0.3), what)
        (r1, p1, _), (r2, p2, _) = TK.rocch_lists_dev(eng, dt, dn_), RC.rocch_from_lists(eng, ht, hn)
        assert r1 == r2 and np.array_equal(p1.vertices, p2.vertices) and np.array_equal(p1.llr.view(np.uint64), p2.llr.view(np.uint64)), what
        # K = 2 systems partitioned with one key: aligned lists
        w = [0.8, 0.4]
        _same_fields(TK.fusion_pass_lists_dev(eng, [dt, dt2], [dn_, dn2], w, 0.1, 0.2), FU.pass_from_lists(eng, [ht, ht2], [hn, hn2], w, 0.1, 0.2), what)
        _same_fields(TK.fusion_fit_lists_dev(eng, [dt, dt2], [dn_, dn2], 0.4), FU.fit_from_lists(eng, [ht, ht2], [hn, hn2], 0.4), what)


def _terms(s, a, c, target):
    """|term| sums of the calibration record's six sums for one class (include/plda_hip.h, "linear score calibration")"""
    s = s.astype(np.float64)
    y = a * s + c
    e = np.exp(-np.abs(y))
    p = np.where(y >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    w = e / (1.0 + e) ** 2
    g = (1.0 - p) if target else p
    L = np.maximum(-y if target else y, 0.0) + np.log1p(e)
    return [np.abs(t).sum() for t in (L, g, g * s, w, w * s, w * s * s)]


def test_rule_all_equals_the_matrix_forms(engines):
    from plda_amd import calibration as CB
    from plda_amd import dcf as DC
    from plda_amd import eer as EE
    from plda_amd import rocch as RC
    from plda_amd import trialkey as TK
    eng = engines[0]
    rng = np.random.default_rng(31)
    m, nt = 67, 1027
    espk, tspk = rng.integers(0, 6, m).astype(np.int64), rng.integers(0, 6, nt).astype(np.int64)
    S = (rng.standard_normal((m, nt)) + 2.0 * (espk[:, None] == tspk[None, :])).astype(np.float32)
    dS, des, dts = _t(S), _t(espk), _t(tspk)
    part = TK.partition_matrix_dev(eng, TK.TrialKey(m, nt, "all"), dS, des, dts)
    tar, non = part.pooled()
    assert tar.data_ptr() == part.tar("all").data_ptr() and tar.shape == part.tar(0).shape
    args = (dS.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr())
    assert np.array_equal(TK.eer_lists_dev(eng, tar, non), EE.eer_from_matrix_dev(eng, *args))
    points = ((0.01, 1.0, 1.0), (0.5, 1.0, 1.0))
    assert TK.min_dcf_lists_dev(eng, tar, non, points)[0] == DC.min_dcf_from_matrix_dev(eng, *args, points=points)[0]
    (r1, p1, _), (r2, p2, _) = TK.rocch_lists_dev(eng, tar, non), RC.rocch_from_matrix_dev(eng, *args)
    assert r1 == r2 and np.array_equal(p1.vertices, p2.vertices)
    a, c, th = 0.9, 0.2, 0.5
    got, ref = TK.calib_pass_lists_dev(eng, tar, non, a, c, th), CB.pass_from_matrix_dev(eng, *args, a=a, c=c, theta=th)
    for k in ("Np", "Nn", "miss", "fa", "nonfinite", "min_t", "max_t", "min_n", "max_n"):
        assert got[k] == ref[k], k
    tgt = espk[:, None] == tspk[None, :]
    for cls, sel in (("t", S[tgt]), ("n", S[~tgt])):
        for name, bound in zip(CB.SUMS, _terms(sel, a, c, cls == "t")):
            k = name + "_" + cls
            print("%s: lists %.17g matrix %.17g bound %.3g" % (k, got[k], ref[k], 2e-12 * bound))
            assert abs(got[k] - ref[k]) <= 2e-12 * bound, k


# ---------------------------------------------------------------------------------------------- end to end
def test_end_to_end_plda_evaluate():
    from conftest import make_data
    from liblda import PLDA
    from plda_amd import calibration as CB
    from plda_amd import dcf as DC
    from plda_amd import eer as EE
    from plda_amd import rocch as RC
    from plda_amd import trialkey as TK
    x, y = make_data(61, 3000, 32, 60, scale_between=0.15)
    p = PLDA(0)
    p.fit(x, y, 5)
    enrol = p.transform(x[:180], y[:180])                                # 60 models of 3 utterances
    test = p.transform(x[1200:1800], np.arange(600, dtype=np.uint64))
    test_speaker = {int(i): int(s) for i, s in zip(range(600), y[1200:1800])}
    p.norm(x[2400:], enrol)
    es = np.array(list(enrol.keys()), np.int64)
    ts = np.array([test_speaker[int(k)] for k in test.keys()], np.int64)
    # a gender-style key: the speaker's parity; a third test label "u" meets enrol label "f" only in speakers enrol lacks
    eg = np.where(es % 2 == 0, "f", "m")
    tg = np.where(ts % 2 == 0, "f", "m")
    tg[:7] = "u"
    rule = {("f", "f"): "female", ("m", "m"): "male", ("m", "u"): "unmatched"}
    ts_map = dict(test_speaker)
    for k in list(test.keys())[:7]:
        ts_map[int(k)] = 1000 + int(k)           # speakers nobody enrolled: "unmatched" has no target
    ts = np.array([ts_map[int(k)] for k in test.keys()], np.int64)
    key = TK.TrialKey(eg, tg, rule)
    points = ((0.01, 1.0, 1.0), (0.05, 1.0, 1.0))
    eng = p._instance if hasattr(p, "_instance") else p
    for kw, S in (({}, p.score_matrix(enrol, test)), ({"znorm": False}, p.score_matrix(enrol, test, znorm=False))):
        got = p.evaluate(enrol, test, ts_map, key, points=points, **kw)
        part = p.partition(enrol, test, ts_map, key, **kw)
        per, tar, non = TM.lists(S, key.enrol_code, key.test_code, key.table, key.n_buckets, es, ts)
        assert got["equalised"]["skipped"] == ["unmatched"] and got["equalised"]["n_buckets"] == 2
        assert got["buckets"]["unmatched"] == {"n_tar": 0, "n_non": len(per[(2, 0)]), "eer": None, "min_dcf": None, "act_dcf": None,
                                               "cllr": None, "min_cllr": None}
        for name, pos, neg in (("female", per[(0, 1)], per[(0, 0)]), ("male", per[(1, 1)], per[(1, 0)]), ("pooled", tar, non)):
            f = got["pooled"] if name == "pooled" else got["buckets"][name]
            if name != "pooled":
                assert np.array_equal(part.tar(name).cpu().numpy().view(np.uint32), TM.bits(pos))
                assert np.array_equal(part.non(name).cpu().numpy().view(np.uint32), TM.bits(neg))
            assert (f["n_tar"], f["n_non"]) == (len(pos), len(neg)) and len(pos) > 0
            assert f["eer"] == EE.eer_from_lists(eng, pos, neg)[3]
            assert f["min_dcf"] == [r["min_dcf"] for r in DC.min_dcf_from_lists(eng, pos, neg, points)[0]]
            assert f["act_dcf"] == [CB.act_dcf(lambda th: CB.pass_from_lists(eng, pos, neg, theta=th), *pt) for pt in points]
            assert f["cllr"] == CB.cllr(CB.pass_from_lists(eng, pos, neg))
            assert f["min_cllr"] == RC.rocch_from_lists(eng, pos, neg)[0]["min_cllr"]
        both = [got["buckets"]["female"], got["buckets"]["male"]]
        eq = got["equalised"]
        for k in ("eer", "cllr", "min_cllr"):
            assert eq[k] == float(np.mean([b[k] for b in both]))
        for k in ("min_dcf", "act_dcf"):
            assert eq[k] == [float(np.mean([b[k][i] for b in both])) for i in range(2)]
    # key=None: every pair, one bucket -- the figures of the whole matrix
    whole = p.evaluate(enrol, test, ts_map, None, points=points)
    S = p.score_matrix(enrol, test)
    tgt = es[:, None] == ts[None, :]
    assert whole["pooled"] == whole["buckets"]["all"] and whole["equalised"]["skipped"] == []
    assert whole["pooled"]["eer"] == EE.eer_from_lists(eng, S[tgt], S[~tgt])[3]
    assert (whole["pooled"]["n_tar"], whole["pooled"]["n_non"]) == (int(tgt.sum()), int((~tgt).sum()))
