"""GPU: VBx's second speaker (plda_vbx_top2[_dev]; csrc/vbx.hip) against its rule (tests/vbx_top2_model.py) applied to the
device's OWN returned gamma, and the six outputs it shares with plda_vbx_dev against that entry, on the bits.

Every plda_vbx_top2_dev call goes through _run2: inputs between NaN (-1) neighbours, every output between guard bands (the
helpers of test_gpu_vbx).  All recordings have D = 8 and run 2 iterations of the (1, 1, 0.9) parameter set: after two, a
speaker that has lost every segment still holds posteriors above those of a far-away one (later its pi underflows)."""
import ctypes as C

import numpy as np
import pytest

import vbx_model as M
import vbx_top2_model as V
from test_gpu_vbx import _assert_same, _bits, _guarded_input, _lib, _Out, _engine, _run, plan_class

pytestmark = pytest.mark.gpu

D = 8
ITERS = 2
PARAMS = M.PARAMS["unit"]


@pytest.fixture(scope="module")
def eng():
    return _engine()


def _run2(eng, recs, phi, want_l2=True, want_p2=True):
    """plda_vbx_top2_dev on guarded buffers -> _run's dict + "labels2" int32 [T], "post2" float64 [T] (None where not asked)"""
    import torch
    from plda_amd import diarize
    y = np.concatenate([np.asarray(r[0], np.float64) for r in recs])
    lab = np.concatenate([np.asarray(r[1], np.int32) for r in recs])
    sizes = np.asarray([len(r[1]) for r in recs], np.int64)
    off = diarize.offsets_of(sizes)
    spk = np.asarray([int(np.max(r[1])) + 1 for r in recs], np.int64)
    goff, poff = diarize.offsets_of(sizes * spk), diarize.offsets_of(spk)
    r, t = len(recs), int(sizes.sum())
    _, dy = _guarded_input(y)
    _, dl = _guarded_input(lab)
    _, dp = _guarded_input(np.asarray(phi, np.float64))
    oL, oK = _Out(t, torch.int32), _Out(r, torch.int32)
    oG, oP = _Out(int(goff[-1]), torch.float64), _Out(int(poff[-1]), torch.float64)
    oE, oI = _Out(r * ITERS, torch.float64), _Out(r, torch.int32)
    oL2, oP2 = _Out(t, torch.int32), _Out(t, torch.float64)
    torch.cuda.synchronize()
    vp = lambda x: C.c_void_p(int(x))
    hp = lambda a: C.c_void_p(a.ctypes.data)
    fa, fb, p = PARAMS
    rc = _lib().plda_vbx_top2_dev(eng._h, vp(dy.data_ptr()), D, vp(dp.data_ptr()), vp(dl.data_ptr()), hp(off), r, float(fa), float(fb),
                                  float(p), 5.0, ITERS, float("-inf"), vp(oL.ptr()), vp(oK.ptr()), vp(oG.ptr()), hp(goff), vp(oP.ptr()),
                                  hp(poff), vp(oE.ptr()), vp(oI.ptr()), vp(oL2.ptr()) if want_l2 else None,
                                  vp(oP2.ptr()) if want_p2 else None)
    torch.cuda.synchronize()
    assert rc == 0, "status %d: %s" % (rc, eng._lib.plda_last_error(eng._h).decode())
    g, pi = oG.check("gamma"), oP.check("pi")
    if not want_l2:
        oL2.check("labels2", written=False)
    if not want_p2:
        oP2.check("post2", written=False)
    return {"labels": oL.check("labels"), "n_clusters": oK.check("n_clusters"),
            "gamma": [g[goff[q]:goff[q + 1]].reshape(int(sizes[q]), int(spk[q])) for q in range(r)],
            "pi": [pi[poff[q]:poff[q + 1]] for q in range(r)], "elbo": oE.check("elbo").reshape(r, ITERS), "iters": oI.check("iters"),
            "labels2": oL2.check("labels2", written=want_l2) if want_l2 else None,
            "post2": oP2.check("post2", written=want_p2) if want_p2 else None}


def _dead_speaker():
    """Three initial labels; the rows of labels 1 and 2 are one and the same vector, six of them with label 1 and five with
    label 2: speaker 1, with more of them, takes every such row, speaker 2 is the runner-up there (1e-2 against 1e-8 for
    speaker 0 after two iterations of tests/vbx_model.py) and nobody's first choice."""
    _, _, _, phi = M.generate(4, D, 1, 1, 0)
    rng = np.random.default_rng(42)
    u, v = rng.standard_normal(D) * np.sqrt(phi), rng.standard_normal(D) * np.sqrt(phi)
    labels = np.asarray([0, 0, 0, 0, 0, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1], np.int32)
    y = np.where((labels == 0)[:, None], u + 0.3 * rng.standard_normal((len(labels), D)), v)
    return y, labels


def _recordings():
    """name -> (y, labels); the shapes of the issue: T x S"""
    hi = M.lds_boundary(D, 10)[1]
    out = {}
    for name, (t, k, s, seed) in {"1x1": (1, 1, 1, 11), "3x2": (3, 2, 2, 12), "70x64": (70, 3, 64, 13), "scratch %dx10" % hi: (hi, 4, 10, 14)}.items():
        y, labels, _, _ = M.generate(t, D, k, s, seed)
        out[name] = (y, labels)
    y, labels, _, _ = M.generate(40, D, 3, 5, 15)
    labels[labels == 2] = 3                                               # label 2 has no segment; S stays 5
    assert 2 not in labels and labels.max() == 4
    out["a label with no segment"] = (y, labels)
    out["a dead speaker"] = _dead_speaker()
    return out


@pytest.fixture(scope="module")
def phi():
    return M.generate(4, D, 1, 1, 0)[3]


@pytest.fixture(scope="module")
def batch(eng, phi):
    """all recordings in one call, computed once and left unchanged"""
    recs = _recordings()
    return recs, _run2(eng, list(recs.values()), phi)


def _check_rule(res, recs, what):
    off = np.concatenate([[0], np.cumsum([len(l) for _, l in recs])])
    for q in range(len(recs)):
        labels, k, labels2, post2 = V.top2(res["gamma"][q])
        a, b = int(off[q]), int(off[q + 1])
        assert np.array_equal(res["labels"][a:b], labels) and int(res["n_clusters"][q]) == k, "%s, recording %d: labels" % (what, q)
        assert np.array_equal(res["labels2"][a:b], labels2), "%s, recording %d: labels2\n%r\n%r" % (what, q, res["labels2"][a:b], labels2)
        assert np.array_equal(_bits(res["post2"][a:b]), _bits(post2)), "%s, recording %d: post2" % (what, q)
        assert ((labels2 >= 0) & (labels2 < k) & (labels2 != labels)).all() if k > 1 else (labels2 == -1).all()


@pytest.mark.parametrize("name", list(_recordings()))
def test_one_recording(eng, phi, batch, name):
    recs, whole = batch
    rec = recs[name]
    t, s = len(rec[1]), int(rec[1].max()) + 1
    one = _run2(eng, [rec], phi)
    _check_rule(one, [rec], name)
    base = _run(eng, [rec], phi, PARAMS, max_iters=ITERS)                 # plda_vbx_dev: the other six outputs, on the bits
    _assert_same(one, dict(base, labels2=None, post2=None), name)
    assert np.array_equal(one["labels"], base["labels"])
    k = int(one["n_clusters"][0])
    if name == "1x1":
        assert k == 1 and one["labels2"].tolist() == [-1] and one["post2"].tolist() == [0.0]
    if name.startswith("scratch"):
        assert plan_class(eng, t, s, D) == 1 and plan_class(eng, t - 1, s, D) == 0 and k >= 2
    if name == "70x64":
        assert s == 64 and k >= 2
    if name == "a dead speaker":
        assert s == 3 and k < s, "the construction must leave a speaker without a first-choice segment"
        g = one["gamma"][0]
        same = rec[1] != 0
        assert (np.argsort(g[same], 1)[:, -2] == 2).all(), "speaker 2 must be the runner-up of the rows it lost"
        assert (one["labels2"][same] == one["labels"][0]).all() and np.array_equal(one["post2"][same], g[same, 0])
    q = list(recs).index(name)                                            # alone = inside the batch, bit for bit
    off = np.concatenate([[0], np.cumsum([len(l) for _, l in recs.values()])])
    _assert_same(dict(whole, labels2=None, post2=None), dict(one, labels2=None, post2=None), name, rec=q)
    for key in ("labels", "labels2", "post2"):
        assert np.array_equal(_bits(whole[key][off[q]:off[q + 1]]), _bits(one[key])), "%s: %s alone and in the batch" % (name, key)


def test_batch_follows_the_rule_and_mixes_the_classes(eng, batch):
    recs, whole = batch
    classes = [plan_class(eng, len(l), int(l.max()) + 1, D) for _, l in recs.values()]
    assert sorted(set(classes)) == [0, 1]
    _check_rule(whole, list(recs.values()), "batch")
    assert (whole["n_clusters"] == 1).any() and (whole["n_clusters"] > 1).any()
    assert (whole["post2"] >= 0).all()


def test_each_output_alone(eng, phi, batch):
    recs, whole = batch
    only_p = _run2(eng, list(recs.values()), phi, want_l2=False)
    assert only_p["labels2"] is None and np.array_equal(_bits(only_p["post2"]), _bits(whole["post2"]))
    only_l = _run2(eng, list(recs.values()), phi, want_p2=False)
    assert only_l["post2"] is None and np.array_equal(only_l["labels2"], whole["labels2"])
    neither = _run2(eng, list(recs.values()), phi, want_l2=False, want_p2=False)
    for got in (only_p, only_l, neither):
        _assert_same(dict(got, labels2=None, post2=None), dict(whole, labels2=None, post2=None), "nullable outputs")
        assert np.array_equal(got["labels"], whole["labels"])


def test_host_forms_and_wrappers(eng, phi, batch):
    import torch
    from plda_amd import diarize
    recs, whole = batch
    y = np.concatenate([r[0] for r in recs.values()])
    lab = np.concatenate([r[1] for r in recs.values()])
    off = diarize.offsets_of([len(r[1]) for r in recs.values()])
    fa, fb, p = PARAMS
    kw = dict(Fa=fa, Fb=fb, loop_prob=p, max_iters=ITERS, epsilon=float("-inf"))
    labels, ncl, labels2, post2, info = diarize.vbx(eng, y, off, lab, phi, return_posteriors=True, return_second=True, **kw)
    assert np.array_equal(labels, whole["labels"]) and np.array_equal(ncl, whole["n_clusters"])
    assert np.array_equal(labels2, whole["labels2"]) and np.array_equal(_bits(post2), _bits(whole["post2"]))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(info["gamma"], whole["gamma"]))
    four = diarize.vbx(eng, y, off, lab, phi, return_second=True, **kw)
    assert len(four) == 4 and np.array_equal(four[2], labels2) and np.array_equal(_bits(four[3]), _bits(post2))
    two = diarize.vbx(eng, y, off, lab, phi, **kw)
    assert len(two) == 2 and np.array_equal(two[0], labels)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dy, dphi, dlab = dev(y), dev(np.asarray(phi, np.float64)), dev(lab)
    oL, oK = torch.zeros(len(lab), dtype=torch.int32, device="cuda"), torch.zeros(len(off) - 1, dtype=torch.int32, device="cuda")
    oL2, oP2 = torch.zeros(len(lab), dtype=torch.int32, device="cuda"), torch.zeros(len(lab), dtype=torch.float64, device="cuda")
    eng.vbx_top2_dev(dy.data_ptr(), D, dphi.data_ptr(), dlab.data_ptr(), off, oL.data_ptr(), oK.data_ptr(), oL2.data_ptr(), oP2.data_ptr(), **kw)
    torch.cuda.synchronize()
    assert np.array_equal(oL.cpu().numpy(), labels) and np.array_equal(oL2.cpu().numpy(), labels2)
    assert np.array_equal(_bits(oP2.cpu().numpy()), _bits(post2))
