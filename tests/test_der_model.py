"""CPU: the host model of the diarisation error rate (tests/der_model.py) against brute force and scipy, the ctypes table
of the five entry points, plda_amd/rttm.py, and the argument checks and tie rule of plda_amd/der.py."""
import io

import numpy as np
import pytest

import der_model as M


def test_model_equals_brute_force_on_small_cases():
    rng = np.random.default_rng(17)
    for case in range(400):
        nr, nc = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        if case % 3 == 0:
            C = rng.integers(0, 3, (nr, nc))                  # tie-heavy: values 0, 1, 2
        elif case % 3 == 1:
            C = rng.integers(0, 2, (nr, nc)) * 7              # 0 or 7
        else:
            C = rng.integers(0, 1000, (nr, nc)) * (rng.random((nr, nc)) < 0.6)
        w, col = M.assign(C)
        assert w == M.brute(C), (case, C)
        used = [j for j in col if j >= 0]
        assert len(set(used)) == len(used)
        assert w == sum(int(C[i, j]) for i, j in enumerate(col) if j >= 0)


def test_greedy_trap_is_a_trap():
    C = M.greedy_trap(1)
    assert C.tolist() == [[10, 9], [9, 0]]
    assert M.assign(C)[0] == 18 == M.brute(C)
    C6 = M.greedy_trap(3)
    assert M.assign(C6)[0] == M.brute(C6) == 18 * (1 + 2 + 3)
    # a greedy largest-cell map: strictly worse on both
    for K, want in ((C, 10), (C6, 10 * 6)):
        K = K.copy()
        got = 0
        while K.max() > 0:
            i, j = np.unravel_index(np.argmax(K), K.shape)
            got += int(K[i, j])
            K[i, :] = 0
            K[:, j] = 0
        assert got == want


def test_model_equals_scipy_up_to_64_by_300():
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(23)
    for nr, nc, hi in ((1, 1, 5), (5, 2, 9), (2, 5, 9), (64, 64, 3), (64, 64, 10 ** 6), (64, 1, 4), (1, 300, 50), (64, 300, 2),
                       (64, 300, 2 ** 40), (33, 257, 1000)):
        C = rng.integers(0, hi, (nr, nc), dtype=np.int64)
        rows, cols = opt.linear_sum_assignment(C, maximize=True)
        assert M.assign(C)[0] == int(C[rows, cols].sum()), (nr, nc, hi)


def test_counts_of_a_worked_example():
    #        ref   0  0  1  1 -1 -1  2
    #        hyp   5  5  5  9  9 -1 -1
    ref = np.asarray([0, 0, 1, 1, -1, -1, 2], np.int32)
    hyp = np.asarray([5, 5, 5, 9, 9, -1, -1], np.int32)
    dur = np.asarray([3, 1, 2, 4, 6, 8, 5], np.int32)
    counts, m, C, rl, hl = M.score_one(ref, hyp, dur)
    assert (rl, hl) == ([0, 1, 2], [5, 9])
    assert C.tolist() == [[4, 0], [2, 4], [0, 0]]
    assert counts == [15, 5, 6, 2] and m == {0: 5, 1: 9}
    assert M.score_one(ref, hyp)[0] == [5, 1, 1, 1]
    row = np.full(64, -1, np.int32)
    row[0], row[1] = 5, 9
    assert M.check_map(row, ref, hyp, dur) == 8
    row[2] = 9
    with pytest.raises(AssertionError):
        M.check_map(row, ref, hyp, dur)


def test_signatures_of_the_five_entry_points():
    from plda_amd import _native as N
    want = {"plda_der_plan": 4, "plda_der_dev": 8, "plda_der": 8, "plda_der_sweep_dev": 13, "plda_der_sweep": 13}
    for name, nargs in want.items():
        assert name in N.SIGNATURES, name
        assert len(N.SIGNATURES[name][1]) == nargs, name


# ------------------------------------------------------------------------------------------- rttm
def test_rttm_round_trip_and_run_merging():
    from plda_amd import rttm
    #                 rec a: 0 0 | gap | 0 1 1 -1 1        rec b: 2
    offsets = np.asarray([0, 7, 8])
    labels = np.asarray([0, 0, 0, 1, 1, -1, 1, 2])
    start = np.asarray([0, 150, 400, 550, 700, 850, 1000, 12])
    dur = np.asarray([150, 150, 150, 150, 150, 150, 33, 1])
    f = io.StringIO()
    rttm.write(f, ["a", "b"], offsets, labels, start, dur)
    lines = f.getvalue().splitlines()
    assert lines[0] == "SPEAKER a 1 0.00 3.00 <NA> <NA> spk0 <NA> <NA>"
    assert len(lines) == 5
    got = rttm.read(io.StringIO(f.getvalue()))
    assert got == {"a": [(0, 300, "spk0"), (400, 150, "spk0"), (550, 300, "spk1"), (1000, 33, "spk1")], "b": [(12, 1, "spk2")]}
    # a file on disk, another tick
    g = io.StringIO()
    rttm.write(g, ["a", "b"], offsets, labels, start, dur, tick=0.001)
    assert rttm.read(io.StringIO(g.getvalue()), tick=0.001) == got
    assert rttm.read(io.StringIO("; comment\nSPKR-INFO a 1 <NA> <NA> <NA> unknown spk0 <NA>\n" + f.getvalue())) == got
    with pytest.raises(ValueError):
        rttm.write(io.StringIO(), ["a"], offsets, labels, start, dur)


def test_rttm_file_on_disk(tmp_path):
    from plda_amd import rttm
    path = str(tmp_path / "x.rttm")
    rttm.write(path, ["r"], [0, 2], [3, 3], [10, 20], [10, 5])
    assert rttm.read(path) == {"r": [(10, 15, "spk3")]}


def test_segment_labels_overlap_ties_and_none():
    from plda_amd import rttm
    turns = [(0, 100, "bob"), (100, 100, "alice"), (150, 100, "carol"), (400, 50, "bob")]
    seg_start = np.asarray([0, 50, 150, 240, 300, 390, 95])
    seg_dur = np.asarray([50, 100, 50, 20, 50, 20, 10])
    labels, names = rttm.segment_labels(turns, seg_start, seg_dur)
    assert names == ["alice", "bob", "carol"]
    #  [0,50) bob; [50,150) bob 50 = alice 50 -> alice (sorted first); [150,200) alice 50 = carol 50 -> alice;
    #  [240,260) carol 10; [300,350) nobody; [390,410) bob 10; [95,105) bob 5 = alice 5 -> alice
    assert labels.tolist() == [1, 0, 0, 2, -1, 1, 0]
    assert labels.dtype == np.int32
    labels, names = rttm.segment_labels([], [0, 5], [5, 5])
    assert labels.tolist() == [-1, -1] and names == []
    with pytest.raises(ValueError):
        rttm.segment_labels([(0, 1, "s%d" % k) for k in range(65)], [0], [1])


# ------------------------------------------------------------------------------------------- der.py without a device
class _NoEngine:
    """an engine whose use is an error: the checks must raise before any device work"""

    def __getattr__(self, name):
        raise AssertionError("the device was touched (%s)" % name)


def test_der_argument_checks_raise_before_any_device_work():
    from plda_amd import der
    e = _NoEngine()
    ok = dict(ref=[0, 1, -1], hyp=[0, 0, 3], offsets=[0, 2, 3])
    bad = [dict(ok, offsets=[0]), dict(ok, offsets=[1, 2, 3]), dict(ok, offsets=[0, 0, 3]), dict(ok, offsets=[0, 3, 2]),
           dict(ok, offsets=[0, 3 + 4097, 3 + 4098]), dict(ok, ref=[0, 64, 0]), dict(ok, ref=[0, -2, 0]), dict(ok, hyp=[0, 4096, 0]),
           dict(ok, hyp=[-2, 0, 0]), dict(ok, ref=[0, 1]), dict(ok, hyp=[[0, 1, 2]]), dict(ok, ref=[0.0, 1.0, 2.0]),
           dict(ok, dur=[1, -1, 1]), dict(ok, dur=[1, 1]), dict(ok, dur=[1.5, 1, 1]), dict(ok, dur=[1, 2 ** 31, 1])]
    for kw in bad:
        with pytest.raises(ValueError):
            der.der(e, **kw)
    merges = (np.zeros(1, np.int32), np.ones(1, np.int32), np.zeros(1))
    sok = dict(merges=merges, offsets=[0, 2, 3], ref=[0, 1, -1], thresholds=[0.0, 1.0])
    sbad = [dict(sok, thresholds=[]), dict(sok, thresholds=[0.0, float("nan")]), dict(sok, thresholds=[[0.0]]),
            dict(sok, merges=merges[:2]), dict(sok, merges=(merges[0], merges[1], np.zeros(2))), dict(sok, ref=[0, 64, 0]),
            dict(sok, num_speakers=0), dict(sok, num_speakers=[1, 1, 1]), dict(sok, dur=[-1, 0, 0]), dict(sok, offsets=[0, 2, 2])]
    for kw in sbad:
        with pytest.raises(ValueError):
            der.sweep(e, **kw)


def test_rates_pooled_and_the_best_tie_rule():
    from plda_amd import der
    counts = np.asarray([[10, 1, 2, 3], [0, 0, 4, 0], [2 ** 62, 2 ** 61, 0, 0]], np.int64)
    r = der.rates(counts)
    assert r[0] == 0.6 and np.isnan(r[1]) and r[2] == 0.5
    assert der.pooled(counts[:2]) == 1.0                                    # (1 + 2 + 3 + 4) / 10
    assert der.pooled(counts) == (10 + 2 ** 61) / (10 + 2 ** 62)            # Python ints: no int64 wrap
    assert np.isnan(der.pooled(counts[1:2]))
    res = der.DerResult(counts[:2])
    assert res.total == 1.0 and res.map is None and res.der[0] == 0.6
    # best: the lowest pooled DER; equal ones -> the lowest index; no speech never wins
    c = np.zeros((5, 2, 4), np.int64)
    c[:, :, 0] = [[10, 10]] * 5
    c[:, 0, 1] = [5, 3, 3, 4, 3]
    assert der.best_index(c) == 1
    s = der.SweepResult(np.arange(5.0), c, np.zeros((5, 2), np.int32))
    assert s.best == 1 and s.der.tolist() == [0.25, 0.15, 0.15, 0.2, 0.15]
    c[0, :, 0] = 0
    assert der.best_index(c) == 1
    c[2] = [[20, 3, 0, 0], [0, 3, 0, 0]]                                   # 6 / 20 > 3 / 20
    c[1, 0, 1] = 4
    assert der.best_index(c) == 4
    # fractions that differ beyond double precision still order exactly
    big = np.zeros((2, 1, 4), np.int64)
    big[0, 0] = [2 ** 60, 2 ** 59 + 1, 0, 0]
    big[1, 0] = [2 ** 60, 2 ** 59, 0, 0]
    assert der.best_index(big) == 1
