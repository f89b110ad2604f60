"""CPU: the host models of the Jaccard error rate (tests/jer_model.py) against each other, against exhaustion, against
der_overlap_model's counts, and at the examples of include/plda_hip.h."""
import math

import numpy as np
import pytest

import der_model as M
import der_overlap_model as O
import jer_model as J

# ref A [0, 10), B [5, 15) / ref A [0, 100): (recording, counts, jer, the pairs jmap may hold)
EXAMPLES = [
    (O.rec(ts=[0, 5], td=[10, 10], tk=[0, 1], ss=[0], sd=[15], hyp=[3]), [20, 5, 0, 5], [2, 2863311530], ({0: 3}, {1: 3})),
    (O.rec(ts=[0, 5], td=[10, 10], tk=[0, 1], ss=[0, 5, 10], sd=[5, 5, 5], hyp=[3, 3, 8], hyp2=[-1, 8, -1]), [20, 0, 0, 0],
     [2, 8589934592], ({0: 3, 1: 8},)),
    (O.rec(ts=[0], td=[100], tk=[0], ss=[0, 40, 200], sd=[40, 30, 1000], hyp=[3, 8, 3]), [100, 30, 1000, 30], [1, 1288490188], ({0: 8},)),
]


@pytest.mark.parametrize("k", [0, 1, 2])
def test_header_examples(k):
    r, counts, jer, _ = EXAMPLES[k]
    for atoms in (J.atoms_ticks, J.atoms_intervals):
        assert J.score(r, atoms=atoms) == (counts, jer)
        four, C, rt, ht, rl, hl = atoms(r)
        assert J.jer(C, rt, ht, J.best_exhaustive) == jer
    assert O.score_ticks(r)[0] == counts


def test_example_figures():
    _, C, rt, ht, rl, hl = J.atoms_ticks(EXAMPLES[0][0])
    assert (rt, ht, C.tolist(), J.weights(C, rt, ht)) == ([10, 10], [15], [[10], [10]], [[2863311530], [2863311530]])
    assert J.rate(EXAMPLES[0][2]) == pytest.approx(2 / 3, abs=2.0 ** -32) and J.rate(EXAMPLES[1][2]) == 0.0
    _, C, rt, ht, rl, hl = J.atoms_ticks(EXAMPLES[2][0])
    assert (rt, ht, hl, J.weights(C, rt, ht)) == ([100], [1040, 30], [3, 8], [[40 * J.ONE // 1100, 30 * J.ONE // 100]])
    assert J.weights(C, rt, ht) == [[156180628, 1288490188]] and J.rate(EXAMPLES[2][2]) == pytest.approx(0.7, abs=2.0 ** -32)
    assert O.best_map_scipy(C) == 40 and J.best_scipy(J.weights(C, rt, ht))[1] == [1]       # map A -> X, jmap A -> Y
    assert math.isnan(J.rate([0, 0]))


@pytest.fixture(scope="module")
def seeded():
    rng = np.random.default_rng(2222)
    out = []
    for k in range(60):
        n, nt = (1, 0) if k == 0 else (int(rng.integers(1, 25)), int(rng.integers(0, 30)))
        r = O.random_recording(rng, n, nt, n_spk=int(rng.integers(1, 5)), span=int(rng.integers(20, 160)), n_hyp=int(rng.integers(1, 7)),
                               n_uem=int(rng.integers(1, 4)) if k % 4 == 0 else 0)
        if k == 1:
            r["hyp"][:] = -1
            r["hyp2"][:] = -1
        out.append(r)
    return out


@pytest.mark.parametrize("collar, skip", [(0, False), (3, False), (1, True)])
def test_the_two_models_agree_and_equal_exhaustion(seeded, collar, skip):
    some = 0
    for k, r in enumerate(seeded):
        a, b = J.atoms_ticks(r, collar, skip), J.atoms_intervals(r, collar, skip)
        assert a[0] == b[0] and a[1].tolist() == b[1].tolist() and a[2:] == b[2:], "recording %d" % k
        four, C, rt, ht, rl, hl = a
        counts = four[:3] + [four[3] - O.best_map_scipy(C)]
        assert counts == O.score_atoms(r, collar, skip)[0] == O.score_ticks(r, collar, skip)[0], "recording %d" % k
        w = J.weights(C, rt, ht)
        got = J.jer(C, rt, ht)
        assert got == J.jer(C, rt, ht, J.best_exhaustive), "recording %d" % k
        assert got[0] == sum(1 for v in rt if v > 0) and 0 <= got[1] <= got[0] * J.ONE
        if got[0]:
            assert abs(J.rate(got) - J.jer_float(C, rt, ht)) <= 2.0 ** -32 + 1e-12, "recording %d" % k
            some += 0 < got[1] < got[0] * J.ONE
    assert some > 30


def test_segment_form_against_a_turn_per_segment():
    """a segment list IS a time line: segment t becomes [t0, t0 + dur) with a reference turn over it"""
    rng = np.random.default_rng(7)
    for _ in range(20):
        ref, hyp, dur = M.random_case(rng, int(rng.integers(1, 40)), 4, 5)
        start = np.concatenate([[0], np.cumsum(dur)[:-1]])
        sel = ref >= 0
        r = O.rec(start[sel], dur[sel], ref[sel], start, dur, hyp)
        a, b = J.atoms_segments(ref, hyp, dur), J.atoms_intervals(r)
        assert a[0] == b[0]
        rows = [i for i, lab in enumerate(a[4]) if lab in b[4]]              # (a label whose segments are all empty has no turn)
        assert a[1][rows].tolist() == b[1].tolist() and [a[2][i] for i in rows] == b[2] and a[3] == b[3]
        assert J.jer(*a[1:4]) == J.jer(*b[1:4]) == J.jer(*a[1:4], J.best_exhaustive)


def test_python_divisions():
    from plda_amd import der
    jc = np.asarray([[2, 2863311530], [0, 0], [1, 1288490188]], np.int64)
    rates = der.jer_rates(jc)
    assert rates[0] == J.rate(jc[0]) and math.isnan(rates[1]) and rates[2] == J.rate(jc[2])
    assert der.pooled_jer(jc) == (3 * J.ONE - 2863311530 - 1288490188) / (3 * J.ONE)
    assert math.isnan(der.pooled_jer(jc[1:2]))
    assert der.best_jer_index(np.asarray([[[1, 5]], [[0, 0]], [[2, 12]], [[1, 6]]], np.int64)) == 2      # ties: the lowest index
