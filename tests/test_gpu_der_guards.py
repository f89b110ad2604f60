"""GPU: the entry points of the diarisation error rate (csrc/der.hip) between guard bands, on fresh and on poisoned scratch,
and through create -> score -> destroy cycles.  The pattern of tests/test_gpu_guard_bands.py (every output between bands of a
payload that must survive outside and be gone inside; test_gpu_der._run / _run_sweep do that for every call) and of
tests/test_gpu_scratch_poison.py (PLDA_SCRATCH_POISON=1 fills every device allocation of the library with 0xFF bytes: a
kernel that reads scratch nobody wrote turns -1 / NaN into a wrong count)."""
import gc

import numpy as np
import pytest

import der_model as M
from test_gpu_der import E_INVAL, _check, _lib, _mixed_recordings, _run, _run_sweep

pytestmark = pytest.mark.gpu


def _engine(monkeypatch, poison, budget=1 << 20):
    from plda_amd import MPlda
    if poison:
        monkeypatch.setenv("PLDA_SCRATCH_POISON", "1")
    else:
        monkeypatch.delenv("PLDA_SCRATCH_POISON", raising=False)
    monkeypatch.setenv("PLDA_DER_SCRATCH_BYTES", str(budget))
    e = MPlda(0)
    monkeypatch.delenv("PLDA_SCRATCH_POISON", raising=False)
    monkeypatch.delenv("PLDA_DER_SCRATCH_BYTES")
    return e


def _sweep_inputs(eng):
    from plda_amd import diarize
    big = diarize.plan(eng, 1)["lds_max"] + 3
    blocks, ref = [], []
    for q, sizes in enumerate(([1], [5, 8], [big // 2, big - big // 2], [70, 70, 70, 70])):
        S, g = M.planted_block(sizes, 90 + q, noise=0.5)
        blocks.append(S)
        ref.append(g)
    ref = np.concatenate(ref).astype(np.int32)
    ref[::11] = -1
    _, _, merges = diarize.ahc(eng, blocks, None, 1, return_merges=True)
    offsets = diarize.offsets_of([b.shape[0] for b in blocks])
    cost = np.sort(merges[2])
    thresholds = np.asarray([-cost[-1] - 1, -cost[len(cost) // 2], 0.0, -cost[0] + 1, -cost[5]], np.float64)
    return merges, offsets, ref, thresholds


def test_fresh_and_poisoned_scratch_agree(monkeypatch):
    """both entry-point families, device and host forms, a scratch budget that a single launch cannot hold: twice on each
    engine, so that the second call meets the first one's scratch"""
    from plda_amd import MPlda, der, diarize
    res = {}
    for poison in (False, True):
        e = _engine(monkeypatch, poison)
        recs = _mixed_recordings(e, 21, 31)
        offsets = diarize.offsets_of([len(x[0]) for x in recs])
        ref, hyp, dur = (np.concatenate([x[k] for x in recs]) for k in range(3))
        merges, soff, sref, thresholds = _sweep_inputs(e)
        out = []
        for _ in range(2):
            out += list(_check(e, recs, "poison = %r" % poison))
            out += list(_run_sweep(e, merges, soff, sref, thresholds, None, [1, 2, 1, 3]))
        host = der.der(e, ref, hyp, offsets, dur, return_map=True)
        hs = der.sweep(e, merges, soff, sref, thresholds, None, [1, 2, 1, 3])
        out += [host.counts, host.map, hs.counts, hs.n_clusters]
        assert np.array_equal(out[0], host.counts) and np.array_equal(out[1], host.map)
        assert np.array_equal(out[2], hs.counts) and np.array_equal(out[3], hs.n_clusters)
        assert _run(e, np.asarray([64], np.int32), np.asarray([0], np.int32), [0, 1], expect=E_INVAL) == E_INVAL
        e.synchronize()
        res[poison] = out
        del e
    MPlda(0)                       # the switch off again for whatever runs next in this process
    for a, b in zip(res[True], res[False]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(res[False][0], res[False][4]) and np.array_equal(res[False][2], res[False][6])      # the second call


def test_create_score_destroy_gives_back_every_byte():
    """plda_destroy frees the scratch, the launch table and the counters of both entry points"""
    from plda_amd import MPlda, der, diarize
    probe = MPlda(0)
    recs = _mixed_recordings(probe, 8, 32)
    merges, soff, sref, thresholds = _sweep_inputs(probe)
    del probe
    offsets = diarize.offsets_of([len(x[0]) for x in recs])
    ref, hyp, dur = (np.concatenate([x[k] for x in recs]) for k in range(3))
    gc.collect()
    first = _lib().plda_device_bytes_held()
    for cycle in range(10):
        e = MPlda(0)
        der.der(e, ref, hyp, offsets, dur, return_map=True)
        der.sweep(e, merges, soff, sref, thresholds)
        assert _lib().plda_device_bytes_held() > first + (64 << 10)          # (a scratch-class matrix is held between calls)
        del e
        gc.collect()
        held = _lib().plda_device_bytes_held()
        assert held == first, "cycle %d: %d bytes of device memory not given back" % (cycle, held - first)
