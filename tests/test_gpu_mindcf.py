"""GPU: the exact minimum detection cost (csrc/dcf.hip) against the host model tests/mindcf_model.py, bit for bit: value,
counts, rates and threshold; every PLDA_MINDCF_VARIANT arm; the relation to the calibration pass (min_dcf <= act_dcf
bit-wise, the returned threshold reproduces the returned counts); the three sources; refusals; guard bands and poisoned
scratch for the device entry points; the row-sharded form; MPlda.min_dcf / PLDA.min_dcf on a fitted model."""
import numpy as np
import pytest

import mindcf_model as mm

pytestmark = pytest.mark.gpu

ENV = ("PLDA_EER_SLAB_ROWS", "PLDA_SCRATCH_POISON", "PLDA_MINDCF_VARIANT")
GUARD_BYTES = 64 << 10


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _engine(monkeypatch, variant=0, d=0, slab=None, poison=False):
    from plda_amd import MPlda
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    if variant:
        monkeypatch.setenv("PLDA_MINDCF_VARIANT", str(variant))
    if slab:
        monkeypatch.setenv("PLDA_EER_SLAB_ROWS", str(slab))
    if poison:
        monkeypatch.setenv("PLDA_SCRATCH_POISON", "1")
    eng = MPlda(0)
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    if d:
        rng = np.random.default_rng(d)
        q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        eng.set_model(rng.random(d), q * (1.0 + rng.random(d))[:, None], np.sort(0.05 + rng.random(d) * 4.0)[::-1].copy())
    return eng


def _case(name):
    """(scores [m, ld] with the matrix in its first nt columns, nt, enrol speakers, test speakers, points)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    pts = mm.FIVE
    if name == "flat":
        pos, neg = mm.flat_cost_lists()
        s = np.empty((1, 2 * len(pos)), np.float32)
        s[0, 0::2], s[0, 1::2] = pos, neg
        ts = np.zeros(2 * len(pos), np.int64)
        ts[0::2] = 1
        return s, s.shape[1], np.array([1], np.int64), ts, ((0.5, 1.0, 1.0),)
    m, nt, k = (1031, 4099, 12) if name == "ragged" else (513, 1025, 16) if name == "seam" else (1500, 2100, 30)
    ld = nt + 5 if name == "ragged" else 1028 if name == "seam" else nt
    es, ts = rng.integers(0, k, m), rng.integers(0, k, nt)
    if name == "few_targets":
        es[:] = np.arange(m) + 1000; ts[:] = np.arange(nt) + 5000; es[:5] = 7; ts[:5] = 7      # 25 targets only
    tgt = es[:, None] == ts[None, :]
    s = rng.standard_normal((m, ld)).astype(np.float32)
    s[:, :nt] += np.float32(2.0) * tgt
    if name == "ties":
        s = (np.round(s * 8) / 8).astype(np.float32)
    if name == "separable":
        s[:, :nt] = np.clip(s[:, :nt], -3, 3) + np.float32(8.0) * tgt
    return s, nt, es.astype(np.int64), ts.astype(np.int64), pts


def _matrix_call(eng, s, nt, es, ts, pts, off=0):
    """off: the matrix starts that many floats into its buffer (a base pointer off the 16-byte boundary)"""
    from plda_amd import dcf
    dS, des, dts = _t(np.concatenate([np.zeros(off, np.float32), s.ravel()])), _t(es), _t(ts)
    import torch
    torch.cuda.synchronize()
    return dcf.min_dcf_from_matrix_dev(eng, dS.data_ptr() + 4 * off, s.shape[1], s.shape[0], nt, des.data_ptr(), dts.data_ptr(), pts)


def _assert_same(got, ref, what):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        print("%s: min_dcf %.17g miss %d fa %d threshold %.17g | model %.17g %d %d %.17g" % (
            what, g["min_dcf"], g["miss"], g["fa"], g["threshold"], r["min_dcf"], r["miss"], r["fa"], r["threshold"]))
        assert mm.same(g, r), (what, g, r)


@pytest.mark.parametrize("name", ["gauss", "ragged", "ties", "separable", "few_targets", "flat", "seam"])
def test_matrix_and_lists_equal_the_model_under_every_variant(monkeypatch, name):
    """Every arm of PLDA_MINDCF_VARIANT (0: the default, 1: never the lists, 2: two nodes per read) and the list form give
    the model's answer bit for bit; the flat-cost set, which the bound cannot prune, takes several launches per level.
    seam: 513 x 1025 under ld = 1028 (a second column strip of one column) from a base pointer one float off."""
    from plda_amd import dcf
    s, nt, es, ts, pts = _case(name)
    pos, neg = mm.split(s[:, :nt], es, ts)
    ref = mm.model(pos, neg, pts)
    if name == "separable":
        assert all(r["min_dcf"] == 0.0 for r in ref)
    if name == "few_targets":
        assert len(pos) == 25
    infos = {}
    for variant in (0, 1, 2):
        eng = _engine(monkeypatch, variant)
        got, info = _matrix_call(eng, s, nt, es, ts, pts, off=1 if name == "seam" else 0)
        _assert_same(got, ref, "%s matrix variant %d" % (name, variant))
        assert (info["Np"], info["Nn"]) == (len(pos), len(neg)) and info["level_bins"][0] == 1
        infos[variant] = info
        lst, linfo = dcf.min_dcf_from_lists(eng, pos, neg, pts)
        _assert_same(lst, ref, "%s lists variant %d" % (name, variant))
        assert not linfo["lists_used"]
        print(name, variant, info)
    assert not infos[1]["lists_used"]
    if name == "flat":
        assert infos[0]["level_bins"][1] > 8 and infos[0]["level_launches"][1] > 1       # more survivors than slots
        assert infos[2]["level_launches"][1] == (infos[2]["level_bins"][1] + 1) // 2 > 1
        assert infos[2]["level_launches"][1] > infos[0]["level_launches"][1]


@pytest.mark.parametrize("npos,nneg", [(1, 70000), (70000, 1)])
def test_a_list_of_one_against_a_list_of_many(monkeypatch, npos, nneg):
    """One launch of one thread's worth beside one of several workgroups, in either order of the two lists."""
    from plda_amd import dcf
    rng = np.random.default_rng(npos)
    pos = (1.0 + rng.standard_normal(npos)).astype(np.float32)
    neg = (-1.0 + rng.standard_normal(nneg)).astype(np.float32)
    ref = mm.model(pos, neg, mm.FIVE)
    for variant in (0, 2):
        got, info = dcf.min_dcf_from_lists(_engine(monkeypatch, variant), pos, neg, mm.FIVE)
        _assert_same(got, ref, "lists %d + %d variant %d" % (npos, nneg, variant))
        assert (info["Np"], info["Nn"]) == (npos, nneg) and not info["lists_used"]


def _torch_model(S, es, ts, pts):
    """tests/mindcf_model.py:model with the sort and the cumulative counts done by torch on the device, for the input too
    large to sort on the host in the test's time; the float64 expression and the first minimum are the host model's."""
    import torch
    tgt = (es[:, None] == ts[None, :]).reshape(-1)
    u = S.reshape(-1).view(torch.int32).to(torch.int64) & 0xffffffff
    u = torch.where(u == 0x80000000, torch.zeros_like(u), u)
    key = torch.where(u >= 0x80000000, 0xffffffff - u, u + 0x80000000)
    del u
    key, order = torch.sort(key)
    cls = tgt[order]
    del order
    n_pos = int(cls.sum())
    n_neg = key.numel() - n_pos
    cum_t = torch.cumsum(cls.to(torch.int64), 0)
    last = torch.ones_like(cls)
    last[:-1] = key[1:] != key[:-1]
    ends = last.nonzero().reshape(-1)
    del last, cls
    miss = torch.cat([torch.zeros(1, dtype=torch.int64, device=S.device), cum_t[ends]])
    fa = n_neg - torch.cat([torch.zeros(1, dtype=torch.int64, device=S.device), (ends + 1) - cum_t[ends]])
    allk = key[ends].cpu().numpy().astype(np.uint32)
    # the cost on the host, by the model's own expression (torch divides by a scalar through its reciprocal: not the definition)
    miss, fa = miss.cpu().numpy(), fa.cpu().numpy()
    out = []
    for pt in pts:
        v = mm.value(pt, miss, fa, n_pos, n_neg)
        i = int(np.argmin(v))                                  # the first minimum is the lowest cut
        out.append(mm._report(pt, v[i], miss[i], fa[i], n_pos, n_neg, i, allk))
    return out


def test_torch_model_is_the_host_model():
    s, nt, es, ts, pts = _case("ties")
    pos, neg = mm.split(s[:, :nt], es, ts)
    _assert_same(_torch_model(_t(s[:, :nt].copy()), _t(es), _t(ts), pts), mm.model(pos, neg, pts), "torch model")


def test_20000_x_20000_takes_three_reads_and_the_lists(monkeypatch):
    """20 000 x 20 000 Gaussian scores with 200 speakers (2e6 targets) at the two NIST points: level 0, level 1 and the
    append are the only reads of the matrix, the rest happens on the lists, and the answer is the model's bit for bit."""
    import torch
    from plda_amd import dcf
    dev = _dev()
    m = nt = 20000
    g = torch.Generator(device=dev); g.manual_seed(3)
    es = torch.randint(0, 200, (m,), device=dev, generator=g)
    ts = torch.randint(0, 200, (nt,), device=dev, generator=g)
    S = torch.randn((m, nt), dtype=torch.float32, device=dev, generator=g)
    S += 2.5 * (es[:, None] == ts[None, :]).float()
    torch.cuda.synchronize()
    eng = _engine(monkeypatch)
    got, info = dcf.min_dcf_from_matrix_dev(eng, S.data_ptr(), nt, m, nt, es.data_ptr(), ts.data_ptr(), mm.NIST)
    print(info)
    again, _ = dcf.min_dcf_from_matrix_dev(eng, S.data_ptr(), nt, m, nt, es.data_ptr(), ts.data_ptr(), mm.NIST)
    ref = _torch_model(S, es, ts, mm.NIST)
    _assert_same(got, ref, "20000 x 20000")
    _assert_same(again, got, "second call")
    assert info["reads"] == 3 and info["lists_used"], info
    assert info["Np"] + info["Nn"] == m * nt and info["level_trials"][2] < 1e-4 * m * nt


def test_min_dcf_and_the_calibration_pass(monkeypatch):
    """min_dcf <= act_dcf bit-wise at the Bayes threshold and at five random thresholds, and a calibration pass at the
    returned threshold returns the returned miss / fa."""
    from plda_amd import calibration as CB
    s, nt, es, ts, pts = _case("gauss")
    eng = _engine(monkeypatch)
    got, _ = _matrix_call(eng, s, nt, es, ts, pts)
    dS, des, dts = _t(s), _t(es), _t(ts)
    rec_at = lambda th: CB.pass_from_matrix_dev(eng, dS.data_ptr(), s.shape[1], s.shape[0], nt, des.data_ptr(), dts.data_ptr(), theta=th)  # noqa: E731
    rng = np.random.default_rng(5)
    for pt, g in zip(pts, got):
        act = CB.act_dcf(rec_at, pt[0], pt[1], pt[2])
        print("point %r: min_dcf %.17g act_dcf at the Bayes threshold %.17g" % (pt, g["min_dcf"], act))
        assert g["min_dcf"] <= act
        for theta in rng.uniform(-2.0, 5.0, 5):
            rec = rec_at(float(theta))
            assert g["min_dcf"] <= CB.act_dcf(rec, pt[0], pt[1], pt[2])
        rec = rec_at(g["threshold"])
        assert (rec["miss"], rec["fa"]) == (g["miss"], g["fa"]), (pt, g, rec["miss"], rec["fa"])


@pytest.mark.parametrize("mixed,zn,m,nt", [(False, False, 900, 1300), (True, True, 900, 1300), (True, True, 513, 1025)],
                         ids=["False-False", "True-True", "True-True-513x1025"])
def test_operand_form_is_score_matrix_plus_matrix_form(monkeypatch, mixed, zn, m, nt):
    import torch
    from plda_amd import dcf
    d = 48
    eng = _engine(monkeypatch, d=d, slab=256)                  # 900 rows: four slabs; 513 rows: three, the last of one row
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
    mat, _ = dcf.min_dcf_from_matrix_dev(eng, S.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr(), mm.FIVE)
    opr, oinfo = dcf.min_dcf_from_operands_dev(eng, dU.data_ptr(), ptr(dn), nu, m, dV.data_ptr(), nt, des.data_ptr(), dts.data_ptr(),
                                               ptr(dzm), ptr(dzs), mm.FIVE)
    opr2, _ = dcf.min_dcf_from_operands_dev(eng, dU.data_ptr(), ptr(dn), nu, m, dV.data_ptr(), nt, des.data_ptr(), dts.data_ptr(),
                                            ptr(dzm), ptr(dzs), mm.FIVE)
    pos, neg = mm.split(S.cpu().numpy(), es, ts)
    ref = mm.model(pos, neg, mm.FIVE)
    _assert_same(mat, ref, "matrix form")
    _assert_same(opr, ref, "operand form, slabs of 256 rows")
    _assert_same(opr, mat, "operand form against matrix form")
    _assert_same(opr2, opr, "operand form again")
    print(oinfo)


def test_refusals(monkeypatch):
    from plda_amd import dcf
    from plda_amd._native import PldaError
    eng = _engine(monkeypatch)
    s, nt, es, ts, pts = _case("gauss")
    for bad, n_bad in ((np.nan, 3), (np.inf, 1), (-np.inf, 2)):
        t = s.copy()
        t.reshape(-1)[:n_bad * 7:7] = bad
        with pytest.raises(PldaError, match="%d non-finite" % n_bad) as e:
            _matrix_call(eng, t, nt, es, ts, pts)
        assert e.value.code == -1
    with pytest.raises(PldaError, match="at least one target") as e:
        _matrix_call(eng, s, nt, es + 1000, ts, pts)                    # no target trial
    assert e.value.code == -1
    with pytest.raises(PldaError, match="at least one target") as e:
        _matrix_call(eng, s[:1, :1].copy(), 1, es[:1], es[:1], pts)     # no non-target trial
    assert e.value.code == -1
    pos, neg = mm.split(s[:, :nt], es, ts)
    with pytest.raises(PldaError) as e:
        dcf.min_dcf_from_lists(eng, pos, neg[:0], pts)
    assert e.value.code == -1
    for bad_pts in (((0.0, 1.0, 1.0),), ((0.5, -1.0, 1.0),), ((1.0, 1.0, 1.0),)):
        with pytest.raises(PldaError, match="operating points") as e:
            dcf.min_dcf_from_lists(eng, pos, neg, bad_pts)
        assert e.value.code == -1
    with pytest.raises(ValueError):
        dcf.min_dcf_from_lists(eng, pos, neg, ((0.5, 1.0, 1.0),) * 9)
    got, _ = dcf.min_dcf_from_lists(eng, pos, neg, pts)                 # the handle is still usable
    _assert_same(got, mm.model(pos, neg, pts), "after the refusals")


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


def _flat(results, info):
    return dict(v=np.array([[r["min_dcf"], r["threshold"], r["far"], r["frr"]] for r in results]),
                c=np.array([[r["miss"], r["fa"]] for r in results], np.int64),
                i=np.array([info["reads"], info["launches"], int(info["lists_used"])] + info["level_bins"] + info["level_trials"], np.int64))


def _device_cases(eng, nan, variant):
    """The three device entry points on guarded inputs -> dict of arrays."""
    from plda_amd import dcf
    out = {}
    for m, nt, ld in ((3, 5, 7), (257, 1023, 1030), (1003, 1999, 2004)):
        rng = np.random.default_rng(m + nt)
        es, ts = rng.integers(0, 9, m), rng.integers(0, 9, nt)
        es[0] = ts[0] = 0; ts[-1] = 100
        S = (rng.standard_normal((m, nt)) + 2.0 * (es[:, None] == ts[None, :])).astype(np.float32)
        keep = [_guarded(S, nan, ld), _guarded(es.astype(np.int64), nan), _guarded(ts.astype(np.int64), nan)]
        res = dcf.min_dcf_from_matrix_dev(eng, keep[0][1].data_ptr(), ld, m, nt, keep[1][1].data_ptr(), keep[2][1].data_ptr(), mm.FIVE)
        for k, v in _flat(*res).items():
            out["matrix%d_%s" % (m, k)] = v
        res = dcf.min_dcf_from_matrix_comm_dev(eng, keep[0][1].data_ptr(), ld, m, nt, keep[1][1].data_ptr(), keep[2][1].data_ptr(), mm.NIST)
        for k, v in _flat(*res).items():
            out["comm%d_%s" % (m, k)] = v
        pos, neg = mm.split(S, es, ts)
        _assert_same(res[0], mm.model(pos, neg, mm.NIST), "comm form %d x %d" % (m, nt))
    d, m, nt, k = 41, 1003, 1999, 37
    rng = np.random.default_rng(9)
    es, ts = rng.integers(0, k, m), rng.integers(0, k, nt)
    spk = rng.standard_normal((k, d)) * 1.2
    U, V = spk[es] + rng.standard_normal((m, d)), spk[ts] + rng.standard_normal((nt, d))
    n = rng.integers(1, 5, m).astype(np.int32)
    keep = [_guarded(x, nan) for x in (U, V, n, es.astype(np.int64), ts.astype(np.int64))]
    res = dcf.min_dcf_from_operands_dev(eng, keep[0][1].data_ptr(), keep[2][1].data_ptr(), 0, m, keep[1][1].data_ptr(), nt,
                                        keep[3][1].data_ptr(), keep[4][1].data_ptr(), points=mm.FIVE)
    for key, v in _flat(*res).items():
        out["operands_%s" % key] = v
    return out


@pytest.mark.parametrize("variant", [0, 2])
def test_device_entry_points_guards_and_poisoned_scratch(monkeypatch, variant):
    """Inputs with NaN (or -1) in the 64 KiB before and after them and behind every row, against zero neighbours; then
    the same on poisoned device scratch (PLDA_SCRATCH_POISON=1: every allocation of the library filled with 0xFF bytes):
    all four runs bit-identical.  (The calls write host structures only: there is no device output to guard.)"""
    from plda_amd import MPlda
    runs = []
    for poison in (False, True):
        for nan in (True, False):
            eng = _engine(monkeypatch, variant, d=41, slab=256, poison=poison)
            runs.append(_device_cases(eng, nan, variant))
            eng.synchronize()
            del eng
    MPlda(0)                                   # the poison switch off again for whatever runs next in this process
    for other in runs[1:]:
        for k, a in runs[0].items():
            assert np.array_equal(a.view(np.uint8), other[k].view(np.uint8)), k


# ---------------------------------------------------------------------------------------------- sharded
def _dcf_rank(rank, world, port, q):
    import os
    import sys
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import mindcf_model as model
    from plda_amd import MPlda, dcf
    from plda_amd.sharding import init_comm, min_dcf_sharded, shard_rows
    dev = torch.device("cuda", 0)                      # the ranks share the one GPU of the test box
    rng = np.random.default_rng(17)                    # same data on every rank
    m, nt = 301, 2997
    es, ts = rng.integers(0, 9, m), rng.integers(0, 9, nt)
    sc = (rng.standard_normal((m, nt)) + 2.0 * (es[:, None] == ts[None, :])).astype(np.float32)
    spans = [shard_rows(m, 2, 0), shard_rows(m, 2, 1), (m, m)] if world == 3 else [shard_rows(m, world, r) for r in range(world)]
    a, b = spans[rank]
    eng = MPlda(0)
    init_comm(eng, transport="host")
    S = torch.from_numpy(sc[a:b].copy()).to(dev)
    e_l = torch.from_numpy(es[a:b].copy()).to(dev)
    t_all = torch.from_numpy(ts).to(dev)
    out, info = min_dcf_sharded(eng, S, e_l, t_all, model.FIVE)
    full = torch.from_numpy(sc).to(dev)
    e_all = torch.from_numpy(es).to(dev)
    one, one_info = dcf.min_dcf_from_matrix_dev(MPlda(0), full.data_ptr(), nt, m, nt, e_all.data_ptr(), t_all.data_ptr(), model.FIVE)
    ref = model.model(*model.split(sc, es, ts), model.FIVE)
    ok = all(model.same(x, y) for x, y in zip(out, one)) and all(model.same(x, y) for x, y in zip(out, ref))
    ok = ok and info["level_bins"] == one_info["level_bins"] and info["lists_used"] == one_info["lists_used"]
    q.put((rank, bool(ok), [sorted(r.items()) for r in out], info))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_min_dcf_of_a_row_sharded_matrix(world):
    """Row slabs held by different ranks (plda_min_dcf_matrix_comm_dev over the host transport, all ranks on this box's GPU;
    with three ranks one owns no row): the answer of the assembled matrix on one GPU, and the model's, on every rank."""
    import multiprocessing as mp
    import os
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 38500 + (os.getpid() % 2000) + world
    procs = [ctx.Process(target=_dcf_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    print(res[0][3])
    assert [r[1] for r in res] == [True] * world, res
    assert all(r[2] == res[0][2] for r in res)


# ---------------------------------------------------------------------------------------------- end to end
def test_end_to_end_plda_min_dcf():
    from conftest import make_data
    from liblda import PLDA
    from plda_amd import calibration as CB
    x, y = make_data(61, 3000, 32, 60, scale_between=0.15)
    p = PLDA(0)
    p.fit(x, y, 5)
    enrol = p.transform(x[:180], y[:180])                                # 60 models of 3 utterances
    test = p.transform(x[1200:2400], np.arange(1200, dtype=np.uint64))
    test_speaker = {int(i): int(s) for i, s in zip(range(1200), y[1200:2400])}
    p.norm(x[2400:], enrol)
    es = np.array(list(enrol.keys()), np.int64)
    ts = np.array([test_speaker[int(k)] for k in test.keys()], np.int64)
    pts = ((0.01, 1.0, 1.0), (0.05, 1.0, 1.0))
    got, info = p.min_dcf(enrol, test, test_speaker, pts)                # operand form: the matrix is never held
    _assert_same(got, mm.model(*mm.split(p.score_matrix(enrol, test), es, ts), pts), "PLDA.min_dcf")
    raw, _ = p.min_dcf(enrol, test, test_speaker, pts, znorm=False)
    _assert_same(raw, mm.model(*mm.split(p.score_matrix(enrol, test, znorm=False), es, ts), pts), "PLDA.min_dcf, znorm=False")
    cohort = p.transform_array(x[2400:], 1)
    asn, _ = p.min_dcf(enrol, test, test_speaker, pts, cohort=cohort, top_k=100)
    _assert_same(asn, mm.model(*mm.split(p.score_matrix_asnorm(enrol, test, cohort, 100), es, ts), pts), "PLDA.min_dcf, AS-norm")
    with pytest.raises(ValueError, match="stored calibration"):
        p.min_dcf(enrol, test, test_speaker, pts, calibrate=True)
    cal = p.calibrate(enrol, test, test_speaker, prior=0.5)
    mapped = p.score_matrix(enrol, test, calibrate=True)
    cg, _ = p.min_dcf(enrol, test, test_speaker, pts, calibrate=True)
    ref = mm.model(*mm.split(mapped, es, ts), pts)
    _assert_same(cg, ref, "PLDA.min_dcf, calibrated")
    # the calibration loss: actDCF of the calibrated scores at the Bayes threshold minus minDCF, never negative
    pos, neg = mm.split(mapped, es, ts)
    for pt, g in zip(pts, cg):
        theta = CB.bayes_theta(pt[0], pt[1], pt[2])
        rec = {"miss": int(np.sum(pos.astype(np.float64) < theta)), "fa": int(np.sum(neg.astype(np.float64) >= theta)), "Np": len(pos), "Nn": len(neg)}
        assert g["min_dcf"] <= CB.act_dcf(rec, pt[0], pt[1], pt[2])
    assert cal.a > 0
    m = p._instance if hasattr(p, "_instance") else p
    same, _ = m.min_dcf(enrol, test, test_speaker, pts)
    _assert_same(same, got, "MPlda.min_dcf")
