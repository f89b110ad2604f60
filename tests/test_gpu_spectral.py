"""GPU: spectral clustering with auto-tuned pruning (csrc/spectral.hip) against its NumPy model (tests/spectral_model.py).

The graph, the choice of the pruning value and the k-means are exact, so they are compared with array_equal STAGE BY STAGE: the
model's selection applied to the device's own eigenvalues, the model's k-means applied to the device's own embedding.  Only
the eigensolver has a tolerance (the cap tests/test_gpu_eig.py holds the direct method to), and only the end-to-end parity
test needs inputs whose decisions clear a margin; it asserts that margin on the model.

Every device call of this file goes through _run: the scores sit between NaN neighbours, every output between guard bands
filled with a payload that must stay intact outside the output and be gone inside it (the pattern of tests/test_gpu_ahc.py)."""
import ctypes as C
import gc

import numpy as np
import pytest

import spectral_model as M

pytestmark = pytest.mark.gpu

GUARD = 16 << 10           # elements on either side
PAYLOAD = 0x7FC0DEAD
E_INVAL = -1
NAMES = ("labels", "n_clusters", "p_used", "k_gap", "eig", "embed", "deg2")


def _dev():
    import torch
    return torch.device("cuda", 0)


def _guarded_input(a):
    """a 1-D host array inside a device buffer whose neighbours are NaN (floats) or -1"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(GUARD + t.numel() + GUARD, dtype=t.dtype, device=_dev())
    buf.fill_(float("nan") if t.dtype.is_floating_point else -1)
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
        return self.body.data_ptr()

    def check(self, what, written=True):
        w = self.words.cpu().numpy().reshape(-1, self.words_per)
        lo, hi = GUARD, GUARD + self.count
        assert (w[:lo] == np.int32(PAYLOAD)).all() and (w[hi:] == np.int32(PAYLOAD)).all(), "%s: guard band overwritten" % what
        if written:
            left = int((w[lo:hi] == np.int32(PAYLOAD)).all(1).sum())
            assert left == 0, "%s: %d output elements never written" % (what, left)
        else:
            assert (w[lo:hi] == np.int32(PAYLOAD)).all(), "%s: written by a call that must write nothing" % what
        return self.body.cpu().numpy().copy()


def _lib():
    from plda_amd import _native as N
    return N.load()


def _vp(x):
    return C.c_void_p(int(x)) if x else None


def _hp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _outs(t, r, P, ms):
    import torch
    return [_Out(t, torch.int32), _Out(r, torch.int32), _Out(r, torch.int32), _Out(r, torch.int32), _Out(r * P * (ms + 2), torch.float64),
            _Out(t * ms, torch.float64), _Out(t, torch.int32)]


def _collect(outs, r, P, ms, t, optional=True):
    res = {}
    for o, name in zip(outs, NAMES):
        res[name] = o.check(name, written=optional or name in ("labels", "n_clusters"))
    res["eig"] = res["eig"].reshape(r, P, ms + 2)
    res["embed"] = res["embed"].reshape(t, ms)
    return res


def _run(eng, blocks, p_table, ms=8, ns=None, max_iters=20, expect=0, optional=True, raw=None, null_out=None):
    """plda_spectral_matrix_dev on guarded buffers -> a dict of the seven outputs (optional=False: the five nullable ones are not
    passed and must stay untouched), or the status code when expect != 0 (every output's payload must then be intact).  raw: a
    dict overriding arguments of the C call (for the argument errors)."""
    import torch
    from plda_amd import diarize
    scores, block_off, offsets = diarize.pack(blocks)
    r, t = len(blocks), int(offsets[-1])
    table = np.ascontiguousarray(np.broadcast_to(np.asarray(p_table, np.int32), (r, np.asarray(p_table).shape[-1])))
    P = table.shape[1]
    nsa = None if ns is None else np.ascontiguousarray(np.broadcast_to(np.asarray(ns, np.int32), (r,)))
    _, ds = _guarded_input(scores)
    outs = _outs(t, r, P, ms)
    a = {"scores": ds.data_ptr(), "block_off": block_off, "offsets": offsets, "R": r, "p_table": table, "P": P, "ms": ms, "ns": nsa,
         "max_iters": max_iters, "outs": [o.ptr() if (optional or i < 2) else None for i, o in enumerate(outs)]}
    a.update(raw or {})
    if null_out is not None:
        a["outs"][null_out] = None
    torch.cuda.synchronize()
    rc = _lib().plda_spectral_matrix_dev(eng._h, _vp(a["scores"]), _hp(a["block_off"]), _hp(a["offsets"]), int(a["R"]), _hp(a["p_table"]),
                                         int(a["P"]), int(a["ms"]), _hp(a["ns"]), int(a["max_iters"]), *[_vp(o) for o in a["outs"]])
    torch.cuda.synchronize()
    assert rc == expect, "status %d: %s" % (rc, eng._lib.plda_last_error(eng._h).decode())
    if expect:
        for o, name in zip(outs, NAMES):
            o.check(name, written=False)
        return rc
    res = _collect(outs, r, P, ms, t, optional)
    res["offsets"], res["p_table"] = offsets, table
    return res


def _bits_equal(a, b, what=""):
    for name in NAMES:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name, x.shape, y.shape)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s %s: %d of %d differ" % (what, name, int((x != y).sum()), x.size)


def _slice(res, q):
    """recording q of a batch result, as a call on it alone would return it"""
    o = res["offsets"]
    s = slice(int(o[q]), int(o[q + 1]))
    return {"labels": res["labels"][s], "n_clusters": res["n_clusters"][q:q + 1], "p_used": res["p_used"][q:q + 1],
            "k_gap": res["k_gap"][q:q + 1], "eig": res["eig"][q:q + 1], "embed": res["embed"][s], "deg2": res["deg2"][s]}


def _check_staged(res, blocks, ms, ns=None, max_iters=20, spectrum=True):
    """the exact stages of every recording against the model, on the device's own eigenvalues and embedding; spectrum: also
    the eigenvalues and the residual of the embedding against the model's exact Laplacian"""
    o, table = res["offsets"], res["p_table"]
    nsa = None if ns is None else np.broadcast_to(np.asarray(ns), (len(blocks),))
    for q, S in enumerate(blocks):
        n = S.shape[0]
        one = _slice(res, q)
        what = "recording %d (N = %d)" % (q, n)
        if n == 1:
            want = M.spectral(S, table[q], ms)
            for name in NAMES:
                assert np.array_equal(np.asarray(one[name]).ravel(), np.asarray(want[name]).ravel()), (what, name)
            continue
        c = M.similarity(S)
        pos, p_used, k_gap, _ = M.choose(one["eig"][0], n, table[q], ms)
        assert one["p_used"][0] == p_used and one["k_gap"][0] == k_gap, (what, one["p_used"], p_used, one["k_gap"], k_gap)
        assert p_used == min(int(table[q][pos]), n - 1)
        L, deg2 = M.laplacian(M.neighbours_fast(c, p_used))
        assert np.array_equal(one["deg2"], deg2), what
        k = min(int(nsa[q]), n) if nsa is not None and nsa[q] > 0 else k_gap
        U = one["embed"][:, :k]
        assert (one["embed"][:, k:].view(np.uint64) == 0).all(), what + ": the unused columns must be +0.0"
        labels, ncl = M.kmeans(U, max_iters)
        assert one["n_clusters"][0] == ncl and np.array_equal(one["labels"], labels), what
        if not spectrum:
            continue
        have = min(ms + 1, n)
        for e, p in enumerate(table[q]):
            lam = np.linalg.eigvalsh(M.laplacian(M.neighbours_fast(c, int(p)))[0])
            row = one["eig"][0, e]
            cap = 2e-12 * lam[-1]
            assert np.abs(row[:have] - lam[:have]).max() <= cap and abs(row[-1] - lam[-1]) <= cap, (what, e)
            assert np.isinf(row[have:-1]).all() and (row[have:-1] > 0).all(), what
            assert (np.diff(row[:have]) >= 0).all(), what
        lam_n = one["eig"][0, pos, -1]
        resid = np.abs(L @ U - U * one["eig"][0, pos, :k][None, :]).max()
        assert resid <= 2e-11 * lam_n, (what, resid, lam_n)


@pytest.fixture(scope="module")
def eng():
    from plda_amd import MPlda
    return MPlda(0)


def _gauss(n, seed):
    return np.random.default_rng(seed).standard_normal((n, n)).astype(np.float32)


def _prow(n, fractions=(0.1, 0.2, 0.3)):
    return [max(1, min(n - 1, max(2, int(np.ceil(f * n))))) for f in fractions]


FAMILIES = {"planted": lambda n: M.planted(n, 3, 0.4, n)[0], "gaussian": lambda n: _gauss(n, n + 1),
            "levels8": lambda n: M.quantised(n, 8, n + 2), "equal": lambda n: M.all_equal(n)}


# ------------------------------------------------------------------------------------------- 1, 2: exact stages, spectrum
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_exact_stages_and_spectrum(eng, family):
    """deg2, the choice of p and k_gap from the device's eigenvalues, the k-means on the device's embedding: bit for bit; the
    eigenvalues within 2e-12 lambda_N and |L U - U Lambda| within 2e-11 lambda_N.  Ties everywhere in `levels8` and `equal`."""
    sizes = [1, 2, 3, 5, 17, 64, 65, 130]
    blocks = [FAMILIES[family](n) for n in sizes]
    table = np.array([_prow(n) for n in sizes], np.int32)
    res = _run(eng, blocks, table, ms=8)
    _check_staged(res, blocks, 8)
    short = _run(eng, blocks, table, ms=8, optional=False)        # the nullable outputs left out: untouched, same labels
    assert np.array_equal(short["labels"], res["labels"]) and np.array_equal(short["n_clusters"], res["n_clusters"])


def test_forced_speaker_count(eng):
    sizes = [1, 2, 6, 40, 90]
    blocks = [M.planted(n, 3, 0.4, 3 * n)[0] for n in sizes]
    table = np.array([_prow(n) for n in sizes], np.int32)
    ns = [2, 2, 0, 5, 8]
    res = _run(eng, blocks, table, ms=8, ns=ns)
    _check_staged(res, blocks, 8, ns=ns)
    assert res["n_clusters"][0] == 1 and res["n_clusters"][1] == 2
    capped = _run(eng, blocks, table, ms=8, ns=ns, max_iters=1)
    _check_staged(capped, blocks, 8, ns=ns, max_iters=1, spectrum=False)


# ------------------------------------------------------------------------------------------- 3: end-to-end parity
PARITY_SIZES = [2, 3, 17, 32, 33, 64, 65, 100, 160, 161, 208, 209, 224, 225, 256, 257]
PARITY_SEED = {2: 0, 3: 0, 17: 0, 32: 0, 33: 3, 64: 0, 65: 0, 100: 0, 160: 7, 161: 5, 208: 2, 209: 0, 224: 0, 225: 0, 256: 0, 257: 0}
_PARITY = {}


def _parity_case():
    """the planted blocks and the model's results, computed once and left unchanged; the seeds were chosen on the CPU so that
    every size clears the margins (with room to spare: second gap <= 0.8 x the first, winner's r <= 0.9 x the runner-up's)"""
    if not _PARITY:
        blocks, want = [], []
        for n in PARITY_SIZES:
            S, _ = M.planted(n, 1 if n < 4 else 2 + n % 3, 0.4, 7000 + 13 * n + PARITY_SEED[n])
            S.setflags(write=False)
            blocks.append(S)
            want.append(M.spectral(S, _prow(n), max_speakers=8))
        _PARITY["blocks"], _PARITY["want"] = blocks, want
    return _PARITY["blocks"], _PARITY["want"]


def test_end_to_end_parity_on_margin_clear_inputs(eng):
    """labels, n_clusters and p_used equal the model's where the model's decisions clear a margin the eigensolver's error
    cannot cross: an eigenvalue error of 2e-12 lambda_N moves a gap of g lambda_N by at most 4e-12 / g relatively, g >= 1e-3"""
    blocks, want = _parity_case()
    for S, w in zip(blocks, want):
        n = S.shape[0]
        for g in w["gaps"]:
            if len(g) > 1:
                assert g[1] <= (1 - 1e-6) * g[0], "N = %d: the two largest gaps tie" % n
            assert g[0] / (w["eig"][0, -1] + 1e-10) >= 1e-3 or n < 4
        rs = np.sort(np.unique(np.asarray(w["rs"])))
        if len(rs) > 1:
            assert rs[1] >= (1 + 1e-6) * rs[0], "N = %d: the two best pruning values tie" % n
    table = np.array([_prow(S.shape[0]) for S in blocks], np.int32)
    res = _run(eng, blocks, table, ms=8)
    _check_staged(res, blocks, 8, spectrum=False)
    for q, w in enumerate(want):
        one = _slice(res, q)
        what = "N = %d" % blocks[q].shape[0]
        assert one["p_used"][0] == w["p_used"] and one["k_gap"][0] == w["k_gap"], what
        assert one["n_clusters"][0] == w["n_clusters"] and np.array_equal(one["labels"], w["labels"]), what
        assert np.array_equal(one["deg2"], w["deg2"]), what


# ------------------------------------------------------------------------------------------- 4: limits and classes
def test_limits(eng):
    """N = 1; p >= N - 1 (the complete graph: L = N I - J, eigenvalues 0 and N); P = 16 with duplicates; max_speakers 1 and 64"""
    res = _run(eng, [np.zeros((1, 1), np.float32)], [[4, 1]], ms=3)
    assert res["labels"].tolist() == [0] and res["n_clusters"].tolist() == [1] and res["p_used"].tolist() == [0]
    assert res["k_gap"].tolist() == [1] and res["deg2"].tolist() == [0] and res["embed"].tolist() == [[1.0, 0.0, 0.0]]
    assert res["eig"][0].tolist() == [[0.0, np.inf, np.inf, np.inf, 0.0]] * 2
    n = 12
    S = _gauss(n, 3)
    res = _run(eng, [S], [[n - 1, n, 1000]], ms=4)
    _check_staged(res, [S], 4)
    assert res["p_used"].tolist() == [n - 1] and (res["deg2"] == 2 * (n - 1)).all()
    assert np.array_equal(res["eig"][0, 0].view(np.uint64), res["eig"][0, 2].view(np.uint64))
    assert np.abs(res["eig"][0, 0, 1:5] - n).max() <= 2e-12 * n and abs(res["eig"][0, 0, 0]) <= 2e-12 * n
    blocks = [M.planted(50, 3, 0.4, 8)[0], _gauss(21, 4)]
    table = np.array([[5, 9, 5, 12, 9, 49, 60, 5, 7, 7, 12, 3, 3, 9, 49, 2], [20, 20, 3, 3, 3, 5, 20, 99, 4, 4, 4, 4, 4, 4, 4, 4]], np.int32)
    res = _run(eng, blocks, table, ms=8)
    _check_staged(res, blocks, 8)
    for q in range(2):
        pe = np.minimum(table[q], blocks[q].shape[0] - 1)
        for e in range(16):
            firsts = int(np.flatnonzero(pe == pe[e])[0])
            assert np.array_equal(res["eig"][q, e].view(np.uint64), res["eig"][q, firsts].view(np.uint64))
    for ms in (1, 64):
        blocks = [M.planted(70, 4, 0.4, ms)[0], _gauss(30, ms), _gauss(2, ms)]
        table = np.array([_prow(b.shape[0]) for b in blocks], np.int32)
        res = _run(eng, blocks, table, ms=ms)
        _check_staged(res, blocks, ms)
        if ms == 1:
            assert res["k_gap"].tolist() == [1, 1, 1] and res["n_clusters"].tolist() == [1, 1, 1]


def test_both_sides_of_every_plan_boundary(eng):
    """one recording on each side of every boundary plda_spectral_plan reports: the selection kernel's classes (P = 1 keeps the
    larger ones quick) and the k-means' LDS / scratch classes at k = 64 and k = 8"""
    from plda_amd import diarize
    edges, n = [], 1
    while n < M.SPECTRAL_MAX:
        plan = diarize.spectral_plan(eng, n, 1)
        assert plan["select_max"] >= n and diarize.spectral_plan(eng, plan["select_max"], 1)["select_class"] == plan["select_class"]
        edges.append(plan["select_max"])
        n = plan["select_max"] + 1
        if n <= M.SPECTRAL_MAX:
            assert diarize.spectral_plan(eng, n, 1)["select_class"] == 2 * plan["select_class"]
    assert edges[-1] == M.SPECTRAL_MAX and len(edges) >= 2
    sizes = [e + d for e in edges[:-1] for d in (0, 1)]
    blocks = [M.quantised(s, 8, s) if s % 2 else M.planted(s, 4, 0.4, s)[0] for s in sizes]
    table = np.array([[max(2, s // 10)] for s in sizes], np.int32)
    _check_staged(_run(eng, blocks, table, ms=6), blocks, 6)
    for k in (64, 8):
        plan = diarize.spectral_plan(eng, 10, k)
        edge = plan["kmeans_lds_max"]
        assert plan["kmeans_cls"] == 0 and diarize.spectral_plan(eng, edge, k)["kmeans_cls"] == 0
        assert diarize.spectral_plan(eng, edge + 1, k)["kmeans_cls"] == 1
        blocks = [M.planted(edge + d, 5, 0.4, edge + k + d)[0] for d in (0, 1)]
        res = _run(eng, blocks, [[edge // 8]], ms=k, ns=k)
        _check_staged(res, blocks, k, ns=k, spectrum=False)


def test_largest_recording(eng):
    """N = PLDA_SPECTRAL_MAX once, P = 1: eight planted groups"""
    n = M.SPECTRAL_MAX
    S, lab = M.planted(n, 8, 0.3, 2048)
    res = _run(eng, [S], [[60]], ms=16)
    _check_staged(res, [S], 16)
    assert res["n_clusters"].tolist() == [8] and M.same_partition(res["labels"], lab)


def test_argument_errors_write_nothing(eng):
    """every refusal is PLDA_E_INVAL before any device work, the outputs' payload intact"""
    blocks = [_gauss(5, 1), _gauss(9, 2)]
    ok = [[2, 3]]
    bad_off = np.array([0, 5, 5], np.int64)
    big = np.array([0, M.SPECTRAL_MAX + 1], np.int64)
    cases = [("P = 0", {"P": 0}), ("P = 17", {"P": M.SPECTRAL_MAX_P + 1}), ("max_speakers = 0", {"ms": 0}),
             ("max_speakers = 65", {"ms": M.SPECTRAL_MAX_SPK + 1}), ("max_iters = 0", {"max_iters": 0}), ("max_iters = 1001", {"max_iters": 1001}),
             ("p = 0", {"p_table": np.array([[2, 3], [0, 3]], np.int32)}), ("p < 0", {"p_table": np.array([[-1, 3], [2, 3]], np.int32)}),
             ("num_speakers < 0", {"ns": np.array([1, -1], np.int32)}), ("num_speakers > max_speakers", {"ns": np.array([9, 1], np.int32)}),
             ("R = 0", {"R": 0}), ("scores NULL", {"scores": None}), ("offsets NULL", {"offsets": None}), ("block_off NULL", {"block_off": None}),
             ("p_table NULL", {"p_table": None}), ("an empty recording", {"offsets": bad_off}),
             ("offsets[0] != 0", {"offsets": np.array([1, 6, 15], np.int64)}),
             ("a block too small", {"block_off": np.array([0, 24, 24 + 81], np.int64)}),
             ("block_off[0] < 0", {"block_off": np.array([-1, 25, 106], np.int64)})]
    for what, raw in cases:
        assert _run(eng, blocks, ok, expect=E_INVAL, raw=raw) == E_INVAL, what
    import torch
    for missing in (0, 1):                                  # labels, n_clusters
        assert _run(eng, blocks, ok, expect=E_INVAL, null_out=missing) == E_INVAL
    # N = 2049: refused from the offsets alone (the scores pointer is never followed)
    tiny = torch.zeros(16, dtype=torch.float32, device=_dev())
    rc = _run(eng, [_gauss(3, 1)], [[2]], expect=E_INVAL,
              raw={"scores": tiny.data_ptr(), "offsets": big, "block_off": np.array([0, (M.SPECTRAL_MAX + 1) ** 2], np.int64)})
    assert rc == E_INVAL and b"PLDA_SPECTRAL_MAX" in eng._lib.plda_last_error(eng._h)


def test_non_finite_scores_fail_and_write_nothing(eng):
    blocks = [_gauss(6, 1), _gauss(40, 2), _gauss(3, 3)]
    blocks[1][7, 30] = np.nan
    blocks[1][31, 2] = np.inf
    blocks[2][1, 1] = np.nan                                # (the diagonal is never read)
    assert _run(eng, blocks, [[2, 3]], expect=E_INVAL) == E_INVAL
    assert b"2 non-finite" in eng._lib.plda_last_error(eng._h)
    blocks[1][7, 30] = blocks[1][31, 2] = 0.0
    _check_staged(_run(eng, blocks, [[2, 3]]), blocks, 8)


# ------------------------------------------------------------------------------------------- 5: reproducibility and hygiene
def _sweep_blocks():
    rng = np.random.default_rng(424242)
    sizes = [1, 2, 300] + [int(s) for s in rng.integers(1, 301, 21)]
    kinds = (lambda n, s: M.planted(n, 3, 0.4, s)[0], _gauss, lambda n, s: M.quantised(n, 8, s))
    return [kinds[i % 3](n, 900 + i) for i, n in enumerate(sizes)]


def test_batch_independence(eng, monkeypatch):
    """24 recordings, N in [1, 300]: each alone equals itself in the batch on the bits of all seven outputs, also when a small
    scratch budget cuts the batch into many groups, and from run to run"""
    from plda_amd import MPlda
    blocks = _sweep_blocks()
    table = np.array([_prow(b.shape[0]) for b in blocks], np.int32)
    ns = [0, 0, 3] + [0] * 21
    batch = _run(eng, blocks, table, ms=8, ns=ns)
    _bits_equal(_run(eng, blocks, table, ms=8, ns=ns), batch, "second run")
    monkeypatch.setenv("PLDA_AHC_SCRATCH_BYTES", str(48 << 10))
    small = MPlda(0)
    monkeypatch.delenv("PLDA_AHC_SCRATCH_BYTES")
    _bits_equal(_run(small, blocks, table, ms=8, ns=ns), batch, "small budget")
    for q, S in enumerate(blocks):
        one = _run(small if q % 2 else eng, [S], table[q:q + 1], ms=8, ns=ns[q])
        _bits_equal(one, _slice(batch, q), "recording %d alone" % q)


def _model_params(d, seed, psi_scale=1.0):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    return rng.random(d), q * (0.5 + rng.random(d))[:, None], np.sort(rng.random(d) * 3.0 + 0.05)[::-1].copy() * psi_scale


def _operand_case(d=24):
    from plda_amd import diarize
    sizes = [1, 5, 64, 150, 37]
    rng = np.random.default_rng(d)
    spk = rng.standard_normal((4, d)) * 1.5
    vecs = np.concatenate([spk[rng.integers(0, 4, n)] + rng.standard_normal((n, d)) for n in sizes])
    return vecs, diarize.offsets_of(sizes), np.array([_prow(n) for n in sizes], np.int32)


def _run_operands(e, dX, offsets, table, ms=8):
    import torch
    r, t, P = len(offsets) - 1, int(offsets[-1]), table.shape[1]
    outs = _outs(t, r, P, ms)
    torch.cuda.synchronize()
    e.score_spectral_dev(dX.data_ptr(), offsets, table, ms, None, 20, *[o.ptr() for o in outs])
    torch.cuda.synchronize()
    res = _collect(outs, r, P, ms, t)
    res["offsets"], res["p_table"] = offsets, table
    return res


def _scored_blocks(e, dX, offsets):
    """every recording's block as plda_score_matrix_dev writes it (ld_out = N) from the device rows dX"""
    import torch
    blocks = []
    for q in range(len(offsets) - 1):
        n = int(offsets[q + 1] - offsets[q])
        S = torch.full((n, n), float("nan"), dtype=torch.float32, device=_dev())
        x = dX[int(offsets[q]):int(offsets[q + 1])]
        torch.cuda.synchronize()
        e.score_matrix_dev(x.data_ptr(), None, 1, n, x.data_ptr(), n, S.data_ptr(), n)
        e.synchronize()
        blocks.append(S.cpu().numpy())
    return blocks


def test_operand_form_equals_matrix_form_on_scored_blocks(eng, monkeypatch):
    """plda_score_spectral_dev == plda_spectral_matrix_dev on the blocks plda_score_matrix_dev writes, bit for bit; the same
    when a small budget walks the call in several slabs (which scores it twice); the host forms agree"""
    import torch
    from plda_amd import MPlda, diarize
    vecs, offsets, table = _operand_case()
    eng.set_model(*_model_params(24, 3))
    dX = torch.from_numpy(vecs).to(_dev())
    blocks = _scored_blocks(eng, dX, offsets)
    got = _run_operands(eng, dX, offsets, table)
    want = _run(eng, blocks, table, ms=8)
    _bits_equal(got, want, "operand against matrix form")
    _check_staged(got, blocks, 8)
    monkeypatch.setenv("PLDA_AHC_SCRATCH_BYTES", str(64 << 10))
    small = MPlda(0)
    monkeypatch.delenv("PLDA_AHC_SCRATCH_BYTES")
    small.set_model(*_model_params(24, 3))
    _bits_equal(_run_operands(small, dX, offsets, table), want, "operand form in slabs")
    labels, ncl, info = diarize.spectral_vectors(eng, vecs, offsets, p=table, max_speakers=8, return_info=True)
    host = dict(info, labels=labels, n_clusters=ncl)
    _bits_equal(host, want, "host operand form")
    labels, ncl, info = diarize.spectral(eng, blocks, p=table, max_speakers=8, return_info=True)
    _bits_equal(dict(info, labels=labels, n_clusters=ncl), want, "host matrix form")
    bad = vecs.copy()
    bad[70, 3] = np.nan
    with pytest.raises(Exception, match="non-finite"):
        diarize.spectral_vectors(small, bad, offsets, p=table, max_speakers=8)


def _engine(monkeypatch, poison):
    from plda_amd import MPlda
    if poison:
        monkeypatch.setenv("PLDA_SCRATCH_POISON", "1")
    else:
        monkeypatch.delenv("PLDA_SCRATCH_POISON", raising=False)
    monkeypatch.setenv("PLDA_AHC_SCRATCH_BYTES", str(256 << 10))
    e = MPlda(0)
    monkeypatch.delenv("PLDA_SCRATCH_POISON", raising=False)
    monkeypatch.delenv("PLDA_AHC_SCRATCH_BYTES")
    return e


@pytest.mark.parametrize("family", ["matrix", "operand"])
def test_fresh_and_poisoned_scratch_agree(monkeypatch, family):
    import torch
    blocks = _sweep_blocks()[:10]
    table = np.array([_prow(b.shape[0]) for b in blocks], np.int32)
    vecs, offsets, vtable = _operand_case()
    res = {}
    for poison in (False, True):
        e = _engine(monkeypatch, poison)
        if family == "matrix":
            res[poison] = _run(e, blocks, table, ms=8)
        else:
            e.set_model(*_model_params(24, 3))
            res[poison] = _run_operands(e, torch.from_numpy(vecs).to(_dev()), offsets, vtable)
    _bits_equal(res[True], res[False], family)


def test_same_bits_after_other_entry_points(eng):
    """a fresh handle against one that first ran fit, cluster, score_dense and plda_sym_eig (which leave their scratch and the
    eigensolver's workspace behind)"""
    from plda_amd import MPlda
    blocks = _sweep_blocks()[:8]
    table = np.array([_prow(b.shape[0]) for b in blocks], np.int32)
    fresh = _run(MPlda(0), blocks, table, ms=8)
    used = MPlda(0)
    rng = np.random.default_rng(12)
    x = rng.standard_normal((400, 12)) + np.repeat(rng.standard_normal((40, 12)) * 2, 10, 0)
    used.fit(x, np.repeat(np.arange(40, dtype=np.uint64), 10), iters=3)
    off = np.array([0, 150, 400], np.int64)
    used.cluster(x, off, threshold=0.0)
    used.score_dense(x, off, 0.5)
    g = rng.standard_normal((300, 300))
    used.sym_eig(g + g.T)
    _bits_equal(_run(used, blocks, table, ms=8), fresh, "after other entry points")


def test_create_spectral_destroy_gives_back_every_byte():
    from plda_amd import MPlda, diarize
    blocks = [_gauss(30, 1), M.planted(140, 3, 0.4, 2)[0]]
    vecs, offsets, table = _operand_case()
    gc.collect()
    first = _lib().plda_device_bytes_held()
    for cycle in range(10):
        e = MPlda(0)
        diarize.spectral(e, blocks, max_speakers=8)
        e.set_model(*_model_params(24, 3))
        diarize.spectral_vectors(e, vecs, offsets, p=table, max_speakers=8)
        assert _lib().plda_device_bytes_held() > first
        del e
        gc.collect()
        held = _lib().plda_device_bytes_held()
        assert held == first, "cycle %d: %d bytes of device memory not given back" % (cycle, held - first)


# ------------------------------------------------------------------------------------------- 6: Python
def _generate(mean, T, psi, counts, rng):
    """rows from the model's own generative form (tests/test_gpu_ahc.py): x = mean + T^-1 (y_speaker + e)"""
    d = len(mean)
    g = rng.permutation(np.repeat(np.arange(len(counts)), counts))
    y = rng.standard_normal((len(counts), d)) * np.sqrt(psi)
    u = y[g] + rng.standard_normal((len(g), d))
    return mean + u @ np.linalg.inv(T).T, g


def test_python_cluster_and_diarize():
    """method="ahc" is the call without the keyword; method="spectral" recovers a clean planted partition with the speaker
    count found from the eigengap; diarize(method="spectral") runs through VBx; the refusals are ValueErrors"""
    from liblda.plda import PLDA
    from plda_amd import diarize
    d, counts = 24, (12, 16, 20, 22)
    mean, T, psi = _model_params(d, 77, psi_scale=30.0)     # (on the host model every p <= 14 of the default table finds the four)
    p = PLDA(0)
    p._instance.set_model(mean, T, psi)
    rng = np.random.default_rng(78)
    rows, groups = zip(*[_generate(mean, T, psi, counts, rng) for _ in range(4)])
    x = np.concatenate(rows)
    n = sum(counts)
    offsets = diarize.offsets_of([n] * 4)
    plain = p.cluster(x, offsets, 0.0, 4, True)
    keyed = p.cluster(x, offsets, 0.0, 4, True, method="ahc")
    for a, b in zip(plain[:2] + plain[2], keyed[:2] + keyed[2]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    labels, ncl, info = p.cluster(x, offsets, method="spectral", max_speakers=8, return_info=True)
    assert ncl.tolist() == [4] * 4 and info["k_gap"].tolist() == [4] * 4
    for q in range(4):
        assert M.same_partition(labels[q * n:(q + 1) * n], groups[q]), "recording %d" % q
    via = diarize.spectral_vectors(p._instance, p._instance.transform_array(x, 1), offsets, max_speakers=8)
    assert np.array_equal(via[0], labels) and np.array_equal(via[1], ncl)
    forced, fk = p.cluster(x, offsets, method="spectral", num_speakers=2)
    assert fk.tolist() == [2] * 4
    pca = p.cluster(x, offsets, method="spectral", target_energy=0.9, max_speakers=8)
    via = diarize.spectral(p._instance, p.score_dense(x, offsets, 0.9), max_speakers=8)
    assert np.array_equal(pca[0], via[0]) and np.array_equal(pca[1], via[1])
    out = p.diarize(x, offsets, method="spectral", max_speakers=8)
    want = p.resegment(x, offsets, labels)
    assert np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[1])
    assert out[0].shape == labels.shape and ((out[1] >= 1) & (out[1] <= 4)).all()
    with pytest.raises(ValueError, match="threshold"):
        p.cluster(x, offsets, threshold=1.0, method="spectral")
    with pytest.raises(ValueError, match="merge"):
        p.cluster(x, offsets, return_merges=True, method="spectral")
    with pytest.raises(ValueError, match="method"):
        p.cluster(x, offsets, method="kmeans")
    with pytest.raises(ValueError, match="spectral"):
        p.cluster(x, offsets, max_speakers=8)
