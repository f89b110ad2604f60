"""CPU: the NumPy model of recording-dependent PCA before dense PLDA scoring (tests/dense_pca_model.py) checked against
facts that do not depend on it: Kaldi's energy rule on hand-made spectra, the rank cap, the empty spectrum, invariance of the
scores under a rotation inside the retained subspace, equality with the full model's oracle LLR when every direction is kept,
and agreement of the eigh and SVD routes."""
import numpy as np
import pytest

import dense_pca_model as dm
from oracle import plda_oracle_np as onp


def test_energy_rule_is_kaldis_with_its_plus_one():
    # one more than the smallest count whose share exceeds the target
    assert dm.energy_dim([0.6, 0.4], 0.5) == 2
    assert dm.energy_dim([0.6, 0.3, 0.1], 0.7) == 3
    # "<=": a share equal to the target does not stop the loop
    assert dm.energy_dim([0.5, 0.25, 0.25], 0.5) == 3
    assert dm.energy_dim([0.5, 0.25, 0.25], 0.4999) == 2
    # a target no partial sum exceeds: all of them, plus one
    assert dm.energy_dim([0.5, 0.3, 0.2], 0.85) == 4
    assert dm.energy_dim([4.0], 0.1) == 2


def test_retained_dimension_is_capped_by_the_rank():
    assert dm.retained(np.array([0.5, 0.3, 0.2]), 0.85) == 3          # dim = 4, rank 3
    assert dm.retained(np.array([1.0, 1e-13, 0.0]), 0.5) == 1          # dim = 2, rank 1 (1e-13 < 2^-40)
    assert dm.retained(np.array([1.0, 1e-11, 0.0]), 0.5) == 2          # 1e-11 > 2^-40
    assert dm.retained(np.array([0.6, 0.4]), 0.5) == 2


def test_no_variance_gives_dimension_zero_and_a_zero_block():
    rng = np.random.default_rng(1)
    model = dm.random_model(rng, 6)
    assert dm.energy_dim(np.zeros(3), 0.3) == 0 and dm.retained(np.zeros(3), 0.3) == 0
    for x in (rng.standard_normal((1, 6)), np.tile(rng.standard_normal(6), (4, 1))):
        s, d, lam = dm.score_block(model, x, 0.3)
        assert d == 0 and not s.any() and not np.signbit(s).any() and not lam.any()


@pytest.mark.parametrize("n,d,target", [(30, 8, 0.5), (6, 12, 0.7), (50, 10, 0.9)])
def test_scores_do_not_depend_on_the_basis_inside_the_subspace(n, d, target):
    rng = np.random.default_rng(n)
    model = dm.random_model(rng, d)
    x = dm.planted_rows(rng, n, d)
    s, k, _ = dm.score_block(model, x, target)
    assert 2 <= k < d
    rot, _ = np.linalg.qr(rng.standard_normal((k, k)))
    s2, k2, _ = dm.score_block(model, x, target, rot=rot)
    assert k2 == k
    assert np.abs(s - s2).max() <= 1e-12 * np.abs(s).max()


def test_full_dimension_is_the_full_models_oracle_llr():
    rng = np.random.default_rng(2)
    d = 8
    model = dm.random_model(rng, d)
    x = dm.planted_rows(rng, 40, d)
    s, k, _ = dm.score_block(model, x, 0.9999)
    assert k == d
    full = dict(model, offset=-model["transform"] @ model["mean"])
    y = onp.transform_ivector(full, x, 1)
    want = onp.llr_matrix(model["psi"], y, 1, y)
    assert np.abs(s - want).max() <= 1e-11 * np.abs(want).max()
    assert np.abs(dm.full_model_llr(model, x) - want).max() <= 1e-11 * np.abs(want).max()
    assert abs(s[0, 1] - onp.llr_pair(model["psi"], y[0], 1, y[1])) <= 1e-11 * np.abs(want).max()


@pytest.mark.parametrize("n,d,target", [(3, 8, 0.3), (8, 8, 0.5), (65, 72, 0.5), (300, 72, 0.3)])
def test_eigh_and_svd_routes_agree(n, d, target):
    rng = np.random.default_rng(10 * n + d)
    model = dm.random_model(rng, d)
    x = dm.planted_rows(rng, n, d)
    share, gap = dm.margins(dm.pca(x)[0], target)
    assert share >= 1e-6 and gap >= 1e-3
    a, da, la = dm.score_block(model, x, target, "eigh")
    b, db, lb = dm.score_block(model, x, target, "svd")
    assert da == db
    assert np.abs(la - lb).max() <= 1e-13 * la[0]
    assert np.abs(a - b).max() <= 1e-11 * np.abs(a).max()


def test_case_generators_meet_their_margins():
    model, x, offsets = dm.case(12, (1, 2, 40, 9), 16, 0.3)
    for r in range(4):
        share, gap = dm.margins(dm.pca(x[offsets[r]:offsets[r + 1]])[0], 0.3)
        assert share >= 1e-6 and gap >= 1e-3
    model, x, offsets, target = dm.ill_conditioned_case()
    lam = dm.pca(x)[0]
    d = dm.retained(lam, target)
    assert dm.margins(lam, target)[0] >= 1e-6 and lam[d - 1] <= 1e-5 * lam[0] and (d == len(lam) or lam[d - 1] >= 2 * lam[d])


def test_c_abi_table_carries_the_entry_points():
    import ctypes as C
    from plda_amd import _native as N
    lib = C.CDLL(N.SO_PATH)
    for name, nargs in (("plda_dense_pca_plan", 4), ("plda_score_dense_pca_dev", 9), ("plda_score_dense_pca", 9),
                        ("plda_score_dense_pca_ahc_dev", 13), ("plda_score_dense_pca_ahc", 13)):
        assert name in N.SIGNATURES and len(N.SIGNATURES[name][1]) == nargs and hasattr(lib, name), name
    assert N.SIGNATURES["plda_score_dense_pca_dev"][1][4] == C.c_double          # target_energy


def test_python_argument_checks_come_before_any_device_work():
    """dense_pca_args needs no device: a stand-in engine that only knows its dimensions."""
    from plda_amd import diarize

    class Eng:
        def __init__(self, dout, din):
            self.d = (dout, din)

        def dims(self):
            return self.d

    x = np.zeros((6, 8))
    assert diarize.dense_pca_args(Eng(8, 8), x, [0, 2, 6], 0.3)[1].dtype == np.int64
    for eng, xx, off, t in ((Eng(5, 8), x, [0, 6], 0.3), (Eng(513, 513), np.zeros((6, 513)), [0, 6], 0.3), (Eng(8, 8), x, [0, 6], 1.0),
                            (Eng(8, 8), x, [0, 6], None), (Eng(8, 8), x, [1, 6], 0.3), (Eng(8, 8), x, [0, 6, 6], 0.3),
                            (Eng(8, 8), x, [0, 5], 0.3), (Eng(8, 8), np.zeros((6, 7)), [0, 6], 0.3),
                            (Eng(8, 8), np.full((6, 8), np.nan), [0, 6], 0.3)):
        with pytest.raises(ValueError):
            diarize.dense_pca_args(eng, xx, off, t)
