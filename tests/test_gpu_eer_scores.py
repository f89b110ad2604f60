"""EER and DET on non-finite, extreme and single-valued scores (include/plda_hip.h, "equal error rate"):
  1. a NaN of either sign or +-Inf among the trials is refused -- PLDA_E_INVAL, the exact count in the message, nothing
     written to the outputs, the handle usable afterwards -- by every EER and DET entry point and in both EER forms;
  2. the padding columns [Nt, ld) and whatever lies in front of the base pointer are not data;
  3. on finite scores the NumPy restatement (oracle/plda_oracle_np.py) is the specification, and the rates returned are farfrr
     at the threshold returned -- also where the last candidate `s_max + 1e-8` is s_max itself (|s_max| >= 2^27)."""
import ctypes as C

import numpy as np
import pytest

from oracle import plda_oracle_np as onp
from test_gpu_eer import _assert_matrix_eer

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
TINY = float(np.float32(1e-45))                       # the smallest subnormal
KINDS = {"+nan": 0x7FC00000, "-nan": 0xFFC00000, "+inf": 0x7F800000, "-inf": 0xFF800000}
SENTINEL = 0x7FF8DEAD0000BEEF                         # what an output array holds before a call that must not write it


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _sentinel(n):
    a = np.empty(n)
    a.view(np.uint64)[:] = SENTINEL
    return a


def _poke(a, index, kind):
    """the bits of `kind` into element `index` of the flat view of a float32 array (a signed NaN does not survive arithmetic)"""
    a.reshape(-1).view(np.uint32)[index] = KINDS[kind]


def _engine(monkeypatch, **env):
    from plda_amd import MPlda
    for k in ("PLDA_EER_VARIANT", "PLDA_EER_SLAB_ROWS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    e = MPlda(0)
    for k in env:
        monkeypatch.delenv(k)
    return e


@pytest.fixture(scope="module")
def eng():
    from plda_amd import MPlda
    return MPlda(0)


def _refused(eng, rc, who, count, *outs):
    """rc is the status of a raw call: PLDA_E_INVAL with the exact count, and every output still holds the sentinel"""
    from plda_amd import _native as N
    with pytest.raises(N.PldaError) as e:
        N.check(eng._h, rc)
    assert e.value.code == -1, e.value
    assert str(e.value).endswith("%s: %d non-finite score(s) among the trials" % (who, count)), e.value
    for o in outs:
        assert (o.view(np.uint64) == SENTINEL).all(), o
    return str(e.value)


def _raw_eer_lists(eng, pos, neg):
    out = _sentinel(6)
    return eng._lib.plda_eer_lists(eng._h, _vp(pos), pos.shape[0], _vp(neg), neg.shape[0], _vp(out)), out


def _raw_det_lists(eng, pos, neg, n):
    far, frr, thr = _sentinel(n), _sentinel(n), _sentinel(n)
    return eng._lib.plda_det_lists(eng._h, _vp(pos), pos.shape[0], _vp(neg), neg.shape[0], n, _vp(far), _vp(frr), _vp(thr)), far, frr, thr


def _raw_eer_matrix(eng, S, ld, m, nt, des, dts, off=0):
    out = _sentinel(6)
    p = lambda t: C.c_void_p(int(t.data_ptr()))          # noqa: E731
    return eng._lib.plda_eer_matrix_dev(eng._h, C.c_void_p(S.data_ptr() + 4 * off), ld, m, nt, p(des), p(dts), _vp(out)), out


def _raw_det_matrix(eng, S, ld, m, nt, des, dts, n, off=0):
    far, frr, thr = _sentinel(n), _sentinel(n), _sentinel(n)
    p = lambda t: C.c_void_p(int(t.data_ptr()))          # noqa: E731
    return eng._lib.plda_det_matrix_dev(eng._h, C.c_void_p(S.data_ptr() + 4 * off), ld, m, nt, p(des), p(dts), n, _vp(far), _vp(frr),
                                        _vp(thr)), far, frr, thr


def _farfrr_holds(thr, far, frr, pos, neg):
    assert far == (np.asarray(neg, np.float64) >= thr).mean() and frr == (np.asarray(pos, np.float64) < thr).mean(), (thr, far, frr)


# ------------------------------------------------------------------------------------ refusal: the two lists
@pytest.fixture(scope="module")
def gauss_lists():
    rng = np.random.default_rng(sum(map(ord, "gauss")))
    pos, neg = rng.normal(2.0, 1.5, 5000).astype(np.float32), rng.normal(-1.0, 1.0, 200000).astype(np.float32)
    return pos, neg, onp.eer(neg, pos)


def _placements(n):
    """one, two and three elements out of: the first, the last, the one a 256-thread block boundary falls on"""
    return [[0], [n - 1], [256], [255, 256], [0, n - 1], [0, 256, n - 1]]


@pytest.mark.parametrize("kind", ["+nan", "-nan", "+inf", "-inf", "mixed"])
def test_lists_with_a_non_finite_score_are_refused(eng, gauss_lists, kind):
    from plda_amd import eer
    pos0, neg0, ref = gauss_lists
    kinds = [kind] * 3 if kind != "mixed" else ["-nan", "+inf", "-inf"]
    for where in ("pos", "neg", "both"):
        for a, b in zip(_placements(pos0.shape[0]), _placements(neg0.shape[0])):
            pos, neg, count = pos0.copy(), neg0.copy(), 0
            for arr, idx in ((pos, a if where != "neg" else []), (neg, b if where != "pos" else [])):
                for j, i in enumerate(idx):
                    _poke(arr, i, kinds[(j + count) % 3])
                count += len(idx)
            rc, out = _raw_eer_lists(eng, pos, neg)
            _refused(eng, rc, "eer", count, out)
            for n in (2, 100):
                rc, far, frr, thr = _raw_det_lists(eng, pos, neg, n)
                _refused(eng, rc, "det", count, far, frr, thr)
    # the handle is as good as new
    thr, far, frr, e = eer.eer_from_lists(eng, pos0, neg0)
    assert (thr, far, frr, e) == ref


def test_the_non_finite_count_comes_before_the_empty_class(eng):
    """one NaN target and no finite one: the answer is the count, not "need at least one target\""""
    pos, neg = np.zeros(1, np.float32), np.arange(4, dtype=np.float32)
    _poke(pos, 0, "-nan")
    rc, out = _raw_eer_lists(eng, pos, neg)
    _refused(eng, rc, "eer", 1, out)
    import torch
    dev = torch.device("cuda", 0)
    S = torch.from_numpy(np.array([[np.inf, -np.inf, np.nan]], np.float32)).to(dev)     # targets only, all of them non-finite
    ids = torch.zeros(3, dtype=torch.int64, device=dev)
    rc, out = _raw_eer_matrix(eng, S, 3, 1, 3, ids, ids)
    _refused(eng, rc, "eer", 3, out)
    rc, far, frr, thr = _raw_det_matrix(eng, S, 3, 1, 3, ids, ids, 2)
    _refused(eng, rc, "det", 3, far, frr, thr)


# ------------------------------------------------------------------------------------ refusal: the matrix, three passes
def _ragged(m, nt, ld, k, off, pad=None, quantised=True):
    """the matrix of test_eer_of_ragged_matrices (quantised Gaussians, a padded and possibly unaligned layout): host scores
    [m, ld], the flat host buffer with `off` floats in front, the labels, the class mask.  pad: the bit patterns that fill the
    padding columns and the floats in front instead."""
    rng = np.random.default_rng(m * 7919 + nt)
    es = rng.integers(0, k, m); ts = rng.integers(0, k, nt)
    es[0] = ts[0] = 0
    ts[-1] = 1; es[-1] = 0
    tgt = es[:, None] == ts[None, :]
    Sh = (rng.standard_normal((m, ld)) * 8).astype(np.float32)
    Sh[:, :nt] += 12.0 * tgt
    if quantised:
        Sh = np.round(Sh * 4) / 4
    front = np.zeros(off, np.float32)
    if pad is not None:
        pat = np.array(pad, np.uint32).view(np.float32)
        Sh[:, nt:] = pat[np.arange(m * (ld - nt)) % len(pat)].reshape(m, ld - nt)
        front = pat[np.arange(off) % len(pat)]
    return Sh, np.concatenate([front, Sh.ravel()]), es, ts, tgt


RAGGED = [(3, 5, 7, 2, 0), (257, 1023, 1023, 9, 0), (300, 1025, 1028, 16, 0), (513, 1025, 1028, 16, 1)]
RAGGED_IDS = ["3-5-7", "257-1023-1023", "300-1025-1028", "513-1025-1028-off1"]


@pytest.mark.parametrize("m,nt,ld,k,off", RAGGED, ids=RAGGED_IDS)
def test_a_matrix_with_a_non_finite_score_is_refused(eng, m, nt, ld, k, off):
    """three-pass form (these shapes are far below the single-pass threshold) and DET: one non-finite trial in the first
    element, the last, the one-column second strip (column 1024), a row that is no multiple of four; then all of them"""
    import torch
    from plda_amd import eer
    dev = torch.device("cuda", 0)
    Sh, flat, es, ts, tgt = _ragged(m, nt, ld, k, off)
    des, dts = torch.from_numpy(es).to(dev), torch.from_numpy(ts).to(dev)
    odd_row = 1 if m < 8 else 101
    spots = [(0, 0), (m - 1, nt - 1), (odd_row, nt // 2)] + ([(odd_row + 1, 1024)] if nt > 1024 else [])
    cases = [([s], kind) for s in spots for kind in KINDS] + [(spots, "-nan"), (spots, "+inf")]
    for where, kind in cases:
        bad = flat.copy()
        for r, c in where:
            _poke(bad, off + r * ld + c, kind)
        S = torch.from_numpy(bad).to(dev)
        rc, out = _raw_eer_matrix(eng, S, ld, m, nt, des, dts, off)
        _refused(eng, rc, "eer", len(where), out)
        rc, far, frr, thr = _raw_det_matrix(eng, S, ld, m, nt, des, dts, 100, off)
        _refused(eng, rc, "det", len(where), far, frr, thr)
    S = torch.from_numpy(flat).to(dev)
    out = eer.eer_from_matrix_dev(eng, S.data_ptr() + 4 * off, ld, m, nt, des.data_ptr(), dts.data_ptr())
    sub = Sh[:, :nt]
    _assert_matrix_eer(out, onp.eer(sub[~tgt], sub[tgt]), tgt)


def test_the_callback_form_refuses_too(eng):
    """plda_eer_matrix_sharded_dev with a one-rank reduction (nothing to add): the same refusal, the same result"""
    import torch
    from plda_amd import eer
    dev = torch.device("cuda", 0)
    m, nt, ld, k, off = RAGGED[2]
    Sh, flat, es, ts, tgt = _ragged(m, nt, ld, k, off)
    des, dts = torch.from_numpy(es).to(dev), torch.from_numpy(ts).to(dev)
    calls = []
    proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint), C.POINTER(C.c_uint))
    cb = proto(lambda ctx, hist, below, above: calls.append(bool(hist)) or 0)

    def call(S):
        out = _sentinel(6)
        p = lambda t: C.c_void_p(int(t.data_ptr()))          # noqa: E731
        return eng._lib.plda_eer_matrix_sharded_dev(eng._h, p(S), ld, m, nt, p(des), p(dts), C.cast(cb, C.c_void_p), None, _vp(out)), out

    bad = flat.copy()
    _poke(bad, 7 * ld + 3, "-inf"); _poke(bad, 299 * ld + 1024, "+nan")
    rc, out = call(torch.from_numpy(bad).to(dev))
    _refused(eng, rc, "eer", 2, out)
    assert calls == [True, True, True, False], calls         # a refusing rank makes the calls its peers wait in
    S = torch.from_numpy(flat).to(dev)
    del calls[:]
    rc, out = call(S)
    assert rc == 0 and calls == [True, True, True, False], calls
    assert np.array_equal(out, eer.eer_from_matrix_dev(eng, S.data_ptr(), ld, m, nt, des.data_ptr(), dts.data_ptr()))
    # a largest score of 2^27 or more: two more passes, each with its reduction, find the largest key
    big = Sh.copy()
    big[:, :nt][tgt] = 3e8
    S = torch.from_numpy(big).to(dev)
    del calls[:]
    rc, out = call(S)
    assert rc == 0 and calls == [True] * 5 + [False], calls
    assert np.array_equal(out, eer.eer_from_matrix_dev(eng, S.data_ptr(), ld, m, nt, des.data_ptr(), dts.data_ptr()))
    sub = big[:, :nt]
    ref = onp.eer(sub[~tgt], sub[tgt])
    assert ref == (3e8, 0.0, 0.0, 0.0)
    _assert_matrix_eer(out, ref, tgt)


# ------------------------------------------------------------------------------------ refusal: the single-pass form
def _poke_dev(S, row, col, kind):
    """the same on a 2-D device tensor; returns what to call to put the old score back.  (The engines run on streams of their
    own: torch's write must have landed before they read.)"""
    import torch
    bits = KINDS[kind]
    cell = S.view(torch.int32)[row, col:col + 1]
    old = cell.clone()
    cell.fill_(bits - (1 << 32) if bits >= (1 << 31) else bits)
    torch.cuda.synchronize()

    def restore():
        cell.copy_(old)
        torch.cuda.synchronize()
    return restore


SINGLE_PASS = {"1500-2100": (1500, 2100, 2100, 30), "ragged": (1031, 4099, 4104, 12),
               # below M Nt = 2^23 the lists' minimum capacity is "too wide a window": the pilot runs, the window pass never does.
               # These two are the smallest at which it does -- 16-byte loads, and scalar ones with a last strip of 3 columns
               "window": (4000, 4100, 4100, 30), "window_ragged": (4001, 4099, 4101, 30)}


@pytest.mark.parametrize("case", list(SINGLE_PASS))
def test_the_single_pass_form_counts_what_its_pilot_does_not_see(monkeypatch, case):
    """PLDA_EER_VARIANT=2 (test_single_pass_eer_forced_on_small_and_awkward_inputs' shapes, and two large enough for the window
    pass to run): the pilot reads every 32nd row, so row 17 is seen by the window pass alone -- whose compares +-Inf pass --
    and row 32 by both.  Refused with count 1 either way, with the message of the three-pass engine; in the window cases the
    refusal of row 17 comes from the window pass itself (no three passes in the trace)."""
    import torch
    dev = torch.device("cuda", 0)
    m, nt, ld, k = SINGLE_PASS[case]
    window = case.startswith("window")
    g = torch.Generator(device=dev); g.manual_seed(sum(map(ord, case)))
    des = torch.randint(0, k, (m,), device=dev, generator=g)
    dts = torch.randint(0, k, (nt,), device=dev, generator=g)
    S = torch.randn((m, ld), dtype=torch.float32, device=dev, generator=g)
    S[:, :nt] += 1.5 * (des[:, None] == dts[None, :]).float()
    torch.cuda.synchronize()
    fast, slow = _engine(monkeypatch, PLDA_EER_VARIANT=2), _engine(monkeypatch, PLDA_EER_VARIANT=1)
    fast.trace_enable(True)
    for row in (17, 32):
        for kind, col in (("+inf", 5), ("-inf", nt - 1), ("+nan", nt // 2), ("-nan", 1024)):
            restore = _poke_dev(S, row, col, kind)
            rc, out = _raw_eer_matrix(fast, S, ld, m, nt, des, dts)
            msg = _refused(fast, rc, "eer", 1, out)
            names = [sp["name"] for sp in fast.trace_read()]
            assert "eer.pilot" in names, names
            if window and row == 17:
                assert "eer.window_pass" in names and "eer.three_passes" not in names, (kind, names)
            rc, out = _raw_eer_matrix(slow, S, ld, m, nt, des, dts)
            assert _refused(slow, rc, "eer", 1, out) == msg
            restore()
    # several, in unsampled rows (the pilot sees finite scores only), beside a padding full of them
    undo = [_poke_dev(S, row, col, list(KINDS)[i % 4]) for i, (row, col) in enumerate([(1, 0), (17, 3), (33, nt - 1), (65, 1024), (m - 1, nt - 1)])]
    if ld > nt:
        pad = S[:, nt:].clone()
        S[:, nt:] = float("inf")
        torch.cuda.synchronize()
    for e in (fast, slow):
        rc, out = _raw_eer_matrix(e, S, ld, m, nt, des, dts)
        _refused(e, rc, "eer", 5, out)
    names = [sp["name"] for sp in fast.trace_read()]
    assert not window or ("eer.window_pass" in names and "eer.three_passes" not in names), names
    for restore in undo:
        restore()
    if ld > nt:
        S[:, nt:] = pad
        torch.cuda.synchronize()
    # finite again: both engines answer, alike; the small cases against the restatement too
    rc, a = _raw_eer_matrix(fast, S, ld, m, nt, des, dts)
    assert rc == 0
    names = [sp["name"] for sp in fast.trace_read()]
    assert not window or ("eer.window_pass" in names and "eer.three_passes" not in names), names
    rc, b = _raw_eer_matrix(slow, S, ld, m, nt, des, dts)
    assert rc == 0
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (a, b)
    assert a[4] + a[5] == m * nt and 0.1 < a[3] < 0.4
    if not window:
        sub, tgt = S[:, :nt].cpu().numpy(), (des[:, None] == dts[None, :]).cpu().numpy()
        _assert_matrix_eer(a, onp.eer(sub[~tgt], sub[tgt]), tgt)


# ------------------------------------------------------------------------------------ refusal: the operand form
@pytest.mark.parametrize("variant", [2, 1], ids=["single_pass", "three_passes"])
def test_the_operand_form_refuses_a_row_of_nans(monkeypatch, variant):
    """plda_score_eer_dev on the seam shape of test_eer_without_the_matrix (513 x 1025, slabs of 256 rows, mixed counts,
    z-norm): a NaN element in the enrol vector of row 512 -- the one-row last slab -- makes that row's 1025 trials NaN.
    Refused with count 1025; with the NaN gone the same handle gives a fresh handle's six numbers bit for bit."""
    import torch
    dev = torch.device("cuda", 0)
    d, m, nt, k = 48, 513, 1025, 40
    rng = np.random.default_rng(sum(map(ord, "seam_windowed")))
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    model = (rng.random(d), q * (1.0 + rng.random(d))[:, None], np.sort(rng.random(d) * 4.0 + 0.05)[::-1].copy())
    es, ts = rng.integers(0, k, m), rng.integers(0, k, nt)
    spk = rng.standard_normal((k, d)) * 1.2
    Uh = spk[es] + rng.standard_normal((m, d))
    V = torch.from_numpy(spk[ts] + rng.standard_normal((nt, d))).to(dev)
    des, dts = torch.from_numpy(es).to(dev), torch.from_numpy(ts).to(dev)
    dn = torch.from_numpy(rng.integers(1, 6, m).astype(np.int32)).to(dev)
    zm = torch.from_numpy(rng.standard_normal(m) * 3.0).to(dev)
    zs = torch.from_numpy(rng.random(m) * 2.0 + 0.5).to(dev)
    p = lambda t: C.c_void_p(int(t.data_ptr()))              # noqa: E731

    def call(e, U):
        out = _sentinel(6)
        return e._lib.plda_score_eer_dev(e._h, p(U), p(dn), 0, m, p(V), nt, p(zm), p(zs), p(des), p(dts), _vp(out)), out

    used = _engine(monkeypatch, PLDA_EER_VARIANT=variant, PLDA_EER_SLAB_ROWS=256)
    fresh = _engine(monkeypatch, PLDA_EER_VARIANT=variant, PLDA_EER_SLAB_ROWS=256)
    used.set_model(*model); fresh.set_model(*model)
    bad = Uh.copy()
    bad[512, 11] = np.nan
    rc, out = call(used, torch.from_numpy(bad).to(dev))
    _refused(used, rc, "eer", 1025, out)
    U = torch.from_numpy(Uh).to(dev)
    rc, again = call(used, U)
    assert rc == 0
    rc, first = call(fresh, U)
    assert rc == 0
    assert np.array_equal(again.view(np.uint64), first.view(np.uint64)), (again, first)
    assert 0.0 < first[3] < 0.45 and first[4] + first[5] == m * nt


# ------------------------------------------------------------------------------------ refusal: the row-sharded form
def _refusing_rank(rank, world, port, q):
    import os
    import sys
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from plda_amd import MPlda, eer
    from plda_amd._native import PldaError
    from plda_amd.sharding import eer_sharded, init_comm, shard_rows
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(17)
    m, nt = 301, 997
    es, ts = rng.integers(0, 9, m), rng.integers(0, 9, nt)
    sc = np.round(rng.standard_normal((m, nt)) + 1.2 * (es[:, None] == ts[None, :]), 2).astype(np.float32)
    spans = [shard_rows(m, 2, 0), shard_rows(m, 2, 1), (m, m)] if world == 3 else [shard_rows(m, world, r) for r in range(world)]
    a, b = spans[rank]
    bad = sc.copy()
    a1, b1 = spans[1]                                    # two non-finite scores, both in rank 1's slab
    bad[a1, 0] = np.nan
    bad[b1 - 1, nt - 1] = -np.inf
    eng = MPlda(0)
    init_comm(eng, transport="host")
    e_l = torch.from_numpy(es[a:b].copy()).to(dev)
    t_all = torch.from_numpy(ts).to(dev)
    code, msg = 0, ""
    try:
        eer_sharded(eng, torch.from_numpy(bad[a:b].copy()).to(dev), e_l, t_all)
    except PldaError as e:
        code, msg = e.code, str(e)
    out = eer_sharded(eng, torch.from_numpy(sc[a:b].copy()).to(dev), e_l, t_all)      # the same engines, finite scores
    full = torch.from_numpy(sc).to(dev)
    e_all = torch.from_numpy(es).to(dev)
    one = MPlda(0)
    ref = eer.eer_from_matrix_dev(one, full.data_ptr(), nt, m, nt, e_all.data_ptr(), t_all.data_ptr())
    # every target at 3e8: the largest key is wanted exactly -- two more passes, each with its reduction, on every rank
    big = sc.copy()
    big[es[:, None] == ts[None, :]] = 3e8
    out_big = eer_sharded(eng, torch.from_numpy(big[a:b].copy()).to(dev), e_l, t_all)
    full_big = torch.from_numpy(big).to(dev)
    ref_big = eer.eer_from_matrix_dev(one, full_big.data_ptr(), nt, m, nt, e_all.data_ptr(), t_all.data_ptr())
    same = bool(np.array_equal(out, ref)) and bool(np.array_equal(out_big, ref_big)) and tuple(ref_big[:4]) == (3e8, 0.0, 0.0, 0.0)
    q.put((rank, code, msg, same, out.tolist() + out_big.tolist()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_every_rank_of_a_sharded_call_refuses_together(world):
    """the harness of test_eer_of_a_row_sharded_matrix: the non-finite scores lie in rank 1's rows only (world 3: rank 2 owns
    none), the count is global, no rank is left waiting in a reduction, and the engines go on to the one-GPU result -- also
    where the largest score is 3e8 and the call makes two more reductions to find it"""
    import multiprocessing as mp
    import os
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 39500 + (os.getpid() % 2000) + world
    procs = [ctx.Process(target=_refusing_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert [r[1] for r in res] == [-1] * world, res
    assert all(r[2].endswith("eer: 2 non-finite score(s) among the trials") for r in res), res
    assert all(r[2] == res[0][2] for r in res), res
    assert [r[3] for r in res] == [True] * world, res
    assert all(r[4] == res[0][4] for r in res)


# ------------------------------------------------------------------------------------ padding is not data
PAD = [KINDS["+nan"], KINDS["+inf"], KINDS["-inf"], KINDS["-nan"], 0x7F7FFFFF]


@pytest.mark.parametrize("m,nt,ld,k,off", [RAGGED[2], RAGGED[3], (1031, 4099, 4104, 12, 0), (1031, 4099, 4104, 12, 3),
                                           (4001, 4099, 4104, 30, 0), (4001, 4099, 4101, 30, 0)],
                         ids=["300-1025-1028", "513-1025-1028-off1", "1031-4099-4104", "1031-4099-4104-off3", "window-4001-4099-4104",
                              "window-4001-4099-4101"])
def test_padding_may_hold_anything(monkeypatch, m, nt, ld, k, off):
    """columns [Nt, ld) and the floats in front of the base pointer full of NaN, +Inf and -Inf: the three-pass EER, the
    single-pass EER (forced) and the DET points are, bit for bit, those of the same matrix with finite padding, and the
    restatement's.  The window cases are large enough for the window pass to run (unquantised scores: it holds the crossing;
    16-byte loads up to a last strip of three columns, and scalar loads), and are held to the three-pass result."""
    import torch
    dev = torch.device("cuda", 0)
    window = m * nt > (1 << 23)
    Sh, clean, es, ts, tgt = _ragged(m, nt, ld, k, off, quantised=not window)
    _, dirty, _, _, _ = _ragged(m, nt, ld, k, off, pad=PAD, quantised=not window)
    assert not np.isfinite(dirty).all() and np.array_equal(dirty.reshape(-1)[off:].reshape(m, ld)[:, :nt], Sh[:, :nt])
    des, dts = torch.from_numpy(es).to(dev), torch.from_numpy(ts).to(dev)
    fast, slow = _engine(monkeypatch, PLDA_EER_VARIANT=2), _engine(monkeypatch, PLDA_EER_VARIANT=1)
    fast.trace_enable(True)
    got = {}
    for name, flat in (("clean", clean), ("dirty", dirty)):
        S = torch.from_numpy(flat).to(dev)
        for e in (fast, slow):
            rc, out = _raw_eer_matrix(e, S, ld, m, nt, des, dts, off)
            assert rc == 0, name
            got.setdefault(name, []).append(out)
        names = [sp["name"] for sp in fast.trace_read()]
        assert "eer.pilot" in names and (not window or ("eer.window_pass" in names and "eer.three_passes" not in names)), names
        rc, far, frr, thr = _raw_det_matrix(slow, S, ld, m, nt, des, dts, 100, off)
        assert rc == 0
        got[name] += [far, frr, thr]
    for a, b in zip(got["clean"], got["dirty"]):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.array_equal(got["dirty"][0].view(np.uint64), got["dirty"][1].view(np.uint64))
    sub = Sh[:, :nt]
    if window:                                             # (the restatement sorts: seconds at this size)
        _farfrr_holds(got["dirty"][0][0], got["dirty"][0][1], got["dirty"][0][2], sub[tgt], sub[~tgt])
        return
    ref = onp.eer(sub[~tgt], sub[tgt])
    _assert_matrix_eer(got["dirty"][0], ref, tgt)
    _assert_matrix_eer(got["dirty"][1], ref, tgt)
    thr_r, far_r, frr_r = onp.det(sub[~tgt], sub[tgt], 100)
    assert np.array_equal(got["dirty"][2], far_r) and np.array_equal(got["dirty"][3], frr_r) and np.array_equal(got["dirty"][4], thr_r)


# ------------------------------------------------------------------------------------ extreme finite scores
@pytest.mark.parametrize("m,nt,k", [(257, 1023, 9), (1500, 2100, 30), (4001, 4099, 30)], ids=["257-1023", "1500-2100", "window-4001-4099"])
@pytest.mark.parametrize("case", ["both_classes", "crossed"])
def test_extreme_finite_scores_match_the_restatement(monkeypatch, eng, case, m, nt, k):
    """+-FLT_MAX, the smallest subnormal of both signs and +-0 among ordinary Gaussians, in both classes; "crossed": FLT_MAX
    only among the impostors, -FLT_MAX only among the targets.  List form and the matrix in both EER forms (the forced
    single-pass form gives up after its pilot at 257 x 1023, for want of targets, and at 1500 x 2100, where a list would be an
    eighth of the matrix; at 4001 x 4099 the window pass runs, and is held to the three passes and to farfrr -- the
    restatement sorts, which takes seconds there)."""
    import torch
    from plda_amd import eer
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(sum(map(ord, case)))
    es, ts = rng.integers(0, k, m), rng.integers(0, k, nt)
    tgt = es[:, None] == ts[None, :]
    Sh = rng.standard_normal((m, nt)).astype(np.float32) + (1.5 * tgt).astype(np.float32)
    flat = Sh.reshape(-1)
    ti, ii = np.flatnonzero(tgt.reshape(-1)), np.flatnonzero(~tgt.reshape(-1))
    small = [TINY, -TINY, 0.0, -0.0]
    t_vals = small + ([FLT_MAX, -FLT_MAX] if case == "both_classes" else [-FLT_MAX, -FLT_MAX])
    i_vals = small + ([FLT_MAX, -FLT_MAX] if case == "both_classes" else [FLT_MAX, FLT_MAX])
    for idx, vals in ((ti, t_vals), (ii, i_vals)):
        where = np.concatenate([idx[:3], idx[-3:], idx[len(idx) // 2:len(idx) // 2 + 6]])      # each value twice: ties at the extremes
        flat[where] = np.array(vals + vals, np.float32)
    pos, neg = Sh[tgt], Sh[~tgt]
    assert (np.abs(pos).max() == FLT_MAX) and (np.abs(neg).max() == FLT_MAX) and (np.abs(Sh)[Sh != 0].min() == TINY)
    S = torch.from_numpy(Sh).to(dev)
    des, dts = torch.from_numpy(es).to(dev), torch.from_numpy(ts).to(dev)
    fast, slow = _engine(monkeypatch, PLDA_EER_VARIANT=2), _engine(monkeypatch, PLDA_EER_VARIANT=1)
    if m * nt > (1 << 23):
        fast.trace_enable(True)
        a = eer.eer_from_matrix_dev(fast, S.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr())
        names = [sp["name"] for sp in fast.trace_read()]
        assert "eer.window_pass" in names and "eer.three_passes" not in names, names
        b = eer.eer_from_matrix_dev(slow, S.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr())
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (a, b)
        assert a[4] == tgt.sum() and a[5] == (~tgt).sum()
        _farfrr_holds(a[0], a[1], a[2], pos, neg)
        return
    ref = onp.eer(neg, pos)
    thr, far, frr, e = eer.eer_from_lists(eng, pos, neg)
    assert (far, frr, e) == ref[1:] and thr == pytest.approx(ref[0], rel=1e-12, abs=1e-300)
    _farfrr_holds(thr, far, frr, pos, neg)
    for en in (fast, slow, eng):
        out = eer.eer_from_matrix_dev(en, S.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr())
        _assert_matrix_eer(out, ref, tgt)
        _farfrr_holds(out[0], out[1], out[2], pos, neg)
    thr_r, far_r, frr_r = onp.det(neg, pos, 100)
    for thr, far, frr in (eer.det_from_lists(eng, pos, neg, 100),
                          eer.det_from_matrix_dev(eng, S.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr(), 100)):
        assert np.array_equal(thr, thr_r) and np.array_equal(far, far_r) and np.array_equal(frr, frr_r)


# ------------------------------------------------------------------------------------ one value, and the collapsing last candidate
@pytest.mark.parametrize("v", [0.25, -0.25, 2.0 ** 26, 2.0 ** 27, 3e8, -3e8, FLT_MAX, 0.0],
                         ids=["0.25", "-0.25", "2^26", "2^27", "3e8", "-3e8", "FLT_MAX", "0"])
def test_single_valued_scores(eng, v):
    """every score equal to v.  The candidates are v and v + 1e-8, the later wins the tie: below 2^27 that is (v + 1e-8, FAR 0,
    FRR 1); from there on v + 1e-8 IS v in float64 and farfrr at v is (FAR 1, FRR 0).  The rates are always farfrr at the
    threshold returned."""
    import torch
    from plda_amd import eer
    dev = torch.device("cuda", 0)
    for npos, nneg in ((1, 1), (3, 5), (70000, 1)):
        pos, neg = np.full(npos, v, np.float32), np.full(nneg, v, np.float32)
        ref = onp.eer(neg, pos)
        out = np.zeros(6)
        from plda_amd import _native as N
        N.check(eng._h, eng._lib.plda_eer_lists(eng._h, _vp(pos), npos, _vp(neg), nneg, _vp(out)))
        print("v = %r, lists (%d, %d): device %r, restatement %r" % (v, npos, nneg, out.tolist(), ref))
        assert tuple(out[1:4]) == ref[1:] and out[0] == pytest.approx(ref[0], rel=1e-12, abs=1e-300), (out, ref)
        assert out[4] == npos and out[5] == nneg
        _farfrr_holds(out[0], out[1], out[2], pos, neg)
        thr, far, frr = eer.det_from_lists(eng, pos, neg, 2)
        thr_r, far_r, frr_r = onp.det(neg, pos, 2)
        assert np.array_equal(thr, thr_r) and np.array_equal(far, far_r) and np.array_equal(frr, frr_r)
    m, nt, ld = 3, 5, 7
    es, ts = np.array([0, 1, 2]), np.array([0, 0, 1, 3, 4])
    tgt = es[:, None] == ts[None, :]
    Sh = np.full((m, ld), v, np.float32)
    Sh[:, nt:] = -1.0                                      # (padding: another value)
    S = torch.from_numpy(Sh).to(dev)
    des, dts = torch.from_numpy(es).to(dev), torch.from_numpy(ts).to(dev)
    out = eer.eer_from_matrix_dev(eng, S.data_ptr(), ld, m, nt, des.data_ptr(), dts.data_ptr())
    sub = Sh[:, :nt]
    ref = onp.eer(sub[~tgt], sub[tgt])
    print("v = %r, matrix: device %r, restatement %r" % (v, out.tolist(), ref))
    _assert_matrix_eer(out, ref, tgt)
    _farfrr_holds(out[0], out[1], out[2], sub[tgt], sub[~tgt])
    thr, far, frr = eer.det_from_matrix_dev(eng, S.data_ptr(), ld, m, nt, des.data_ptr(), dts.data_ptr(), 2)
    thr_r, far_r, frr_r = onp.det(sub[~tgt], sub[tgt], 2)
    assert np.array_equal(thr, thr_r) and np.array_equal(far, far_r) and np.array_equal(frr, frr_r)


BIG = float(np.float32(3e8))
BIG_NEXT = float(np.nextafter(np.float32(3e8), np.float32(np.inf)))
COLLAPSING = {
    # (negatives, positives): the largest score is >= 2^27 in magnitude, so the restatement's last candidate is that score and
    # repeats the rates of the candidate before it -- which it replaces wherever that one wins
    "separable_far_successor": ([1.0, 2.0], [BIG]),                  # the winner's successor is the largest key, far away
    "separable_next_float": ([BIG], [BIG_NEXT]),                     # ... and the very next float
    "inverted": ([BIG], [1.0, 2.0]),
    "crossing_at_the_top": ([1.0, BIG], [BIG]),                      # the earlier candidate wins at the largest key
    "all_negative": ([-2 * BIG, -BIG], [-BIG]),
    "top_not_reached": ([1.0, 2.0, 3.0, BIG], [0.5, 2.5]),           # the crossing lies well below: nothing changes
    "below_2^27": ([1.0, 2.0], [2.0 ** 26]),                         # 2^26 + 1e-8 is a float64 of its own
    "many": (list(np.linspace(-5, 5, 700)) + [BIG] * 3, list(np.linspace(-4, 6, 300)) + [BIG] * 2),
}


@pytest.mark.parametrize("case", list(COLLAPSING))
def test_the_last_candidate_at_a_large_maximum(eng, case):
    neg, pos = (np.array(a, np.float32) for a in COLLAPSING[case])
    from plda_amd import eer
    ref = onp.eer(neg, pos)
    thr, far, frr, e = eer.eer_from_lists(eng, pos, neg)
    print("%s: device %r, restatement %r" % (case, (thr, far, frr, e), ref))
    assert (far, frr, e) == ref[1:] and thr == pytest.approx(ref[0], rel=1e-12, abs=1e-300), ((thr, far, frr, e), ref)
    _farfrr_holds(thr, far, frr, pos, neg)


@pytest.mark.parametrize("top", [BIG, 2.0 ** 26], ids=["3e8", "2^26"])
def test_the_last_candidate_in_both_matrix_forms(monkeypatch, top):
    """4000 x 4100 (the window pass runs), impostors Gaussian, every target equal to `top`: the candidate after the largest
    impostor wins with both rates 0, and its successor is the largest key -- so the answer is known without the restatement:
    that midpoint, or, where top + 1e-8 == top, the last candidate `top` itself, which ties with it.  The window reaches the top
    of the data; the single-pass form must come to the three-pass answer whichever way it goes about it."""
    import torch
    from plda_amd import eer
    dev = torch.device("cuda", 0)
    m, nt, k = 4000, 4100, 100
    g = torch.Generator(device=dev); g.manual_seed(5)
    des = torch.randint(0, k, (m,), device=dev, generator=g)
    dts = torch.randint(0, k, (nt,), device=dev, generator=g)
    S = torch.randn((m, nt), dtype=torch.float32, device=dev, generator=g)
    tgt = des[:, None] == dts[None, :]
    top_imp = float(S[~tgt].max())
    S[tgt] = top
    torch.cuda.synchronize()
    n_tgt = int(tgt.sum())
    thr = top if top + 1e-8 == top else top_imp + (top - top_imp) / 2.0
    assert (top + 1e-8 == top) == (top >= 2.0 ** 27)
    want = np.array([thr, 0.0, 0.0, 0.0, n_tgt, m * nt - n_tgt])
    small = onp.eer([top_imp - 1.0, top_imp], [top, top])       # the same situation in four scores
    assert small == (thr, 0.0, 0.0, 0.0)
    for variant in (1, 2):
        en = _engine(monkeypatch, PLDA_EER_VARIANT=variant)
        en.trace_enable(True)
        out = eer.eer_from_matrix_dev(en, S.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr())
        names = [sp["name"] for sp in en.trace_read()]
        print("top = %r, variant %d: device %r, expected %r, %r" % (top, variant, out.tolist(), want.tolist(), names))
        assert np.array_equal(out, want), (out, want)
        assert variant == 1 or "eer.window_pass" in names, names
