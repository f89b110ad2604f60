"""The embedding chain's NumPy model, its error bound, the host objects around it (EmbeddingChain, Kaldi vector / matrix I/O,
the ctypes table, the npz keys).  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed_model as em  # noqa: E402

from plda_amd import _native as N  # noqa: E402
from plda_amd import kaldi_io  # noqa: E402
from plda_amd.embed import EmbeddingChain, recipe  # noqa: E402

SHAPES = [(1, 1), (2, 1), (7, 15), (16, 16), (17, 17), (200, 150), (256, 200), (520, 512), (512, 513), (2048, 128)]
FORMS = ["kaldi", "vbx", "centre", "bare_A", "A_mout", "len_in_only"]


def make_chain(form, din, dout, rng, offset=0.0):
    """The six chain forms: each of m_in, len_in, A, m_out, len_out is present and absent at least once."""
    m_in = rng.standard_normal(din) + offset
    A = rng.standard_normal((dout, din)) / np.sqrt(din)
    m_out = rng.standard_normal(dout) * 0.1
    if form == "kaldi":
        return em.Chain(m_in, 0.0, A, None, np.sqrt(dout))
    if form == "vbx":
        return em.Chain(m_in, 1.0, A, m_out * 0.1, 1.0)
    if form == "centre":                      # no A: dout = din
        return em.Chain(m_in, 0.0, None, None, np.sqrt(din))
    if form == "bare_A":
        return em.Chain(None, 0.0, A, None, 0.0)
    if form == "A_mout":
        return em.Chain(None, 0.0, A, m_out, 0.0)
    return em.Chain(m_in, 2.0, None, rng.standard_normal(din) * 0.1, 0.0)     # len_in_only


def _apply_reordered(chain, x):
    """The fp64 model with the k-sum (and both norm sums) taken in another order: reversed, pairwise."""
    c2 = em.Chain(None if chain.m_in is None else chain.m_in[::-1].copy(), chain.len_in,
                  None if chain.A is None else np.ascontiguousarray(chain.A[:, ::-1]),
                  chain.m_out[::-1].copy() if chain.A is None and chain.m_out is not None else chain.m_out, chain.len_out)
    out = em.apply(c2, np.ascontiguousarray(x[:, ::-1]))
    return out if chain.A is not None else out[:, ::-1]


@pytest.mark.parametrize("din,dout", SHAPES)
def test_fp64_model_within_a_quarter_of_the_bound(din, dout):
    rng = np.random.default_rng(din * 4099 + dout)
    for form in FORMS:
        for offset in (0.0, 1e3, 1e5):
            for dt in (np.float32, np.float64):
                ch = make_chain(form, din, dout, rng, offset)
                x = (rng.standard_normal((9, din)) + offset).astype(dt)
                ref = em.apply(ch, x, np.longdouble)
                bound = em.error_bound(ch, x)
                for got in (em.apply(ch, x), _apply_reordered(ch, x)):
                    err = np.abs(np.asarray(got, np.longdouble) - ref).astype(np.float64)
                    assert np.all(err <= 0.25 * bound), (form, offset, dt, float(np.max(err / np.maximum(bound, 1e-300))))


def test_recipes_equal_their_compositions():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((11, 24)) + 3.0
    m1, m2 = rng.standard_normal(24), rng.standard_normal(10) * 0.1
    lda = rng.standard_normal((10, 24))
    l2 = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)
    assert np.allclose(em.apply(em.Chain(m1, 1.0, lda, m2, 1.0), x), l2(l2(x - m1) @ lda.T - m2), rtol=1e-13, atol=0)
    t = (x - m1) @ lda.T
    assert np.allclose(em.apply(em.Chain(m1, 0.0, lda, None, np.sqrt(10)), x), t * np.sqrt(10) / np.linalg.norm(t, axis=1, keepdims=True),
                       rtol=1e-13, atol=0)
    c = x - m1
    assert np.allclose(em.apply(em.Chain(m1, 0.0, None, None, np.sqrt(24)), x), c * np.sqrt(24) / np.linalg.norm(c, axis=1, keepdims=True),
                       rtol=1e-13, atol=0)
    assert recipe("vbx") == ("lda", 1.0, 1.0) and recipe("kaldi-lda") == ("lda", 0.0, None)
    assert recipe("kaldi-whiten")[0] == "whiten" and recipe("centre-norm")[0] == "centre"
    with pytest.raises(ValueError):
        recipe("nope")


def test_zero_rows_stay_zero_and_nonfinite_rows_stay_alone():
    rng = np.random.default_rng(4)
    m_in = rng.standard_normal(8)
    ch = em.Chain(m_in, 1.0, rng.standard_normal((5, 8)), None, 1.0)
    x = rng.standard_normal((4, 8))
    x[1] = m_in
    x[2, 3] = np.nan
    out = em.apply(ch, x)
    assert np.all(out[1] == 0) and not np.all(np.isfinite(out[2])) and np.all(np.isfinite(out[[0, 1, 3]]))


def planted(n_spk, d, rng, offset=0.0):
    lab = np.repeat(np.arange(n_spk), rng.integers(3, 13, n_spk))
    wstd = np.linspace(1.0, 2.0, d)
    bstd = np.linspace(3.0, 0.2, d)
    basis = np.linalg.qr(rng.standard_normal((d, d)))[0]
    x = ((rng.standard_normal((n_spk, d)) * bstd)[lab] + rng.standard_normal((len(lab), d)) * wstd) @ basis + offset
    return x, lab


@pytest.mark.parametrize("len_in", [0.0, 1.0])
def test_fit_invariants(len_in):
    rng = np.random.default_rng(5)
    x, lab = planted(40, 12, rng, 2.0)
    ch, lam = em.fit(x, None, 1, 7, len_in, 0.0)
    y = em.apply(ch, x)
    assert np.allclose(y.mean(axis=0), 0, atol=1e-10) and np.allclose(y.T @ y / len(x), np.eye(7), atol=1e-10)
    assert np.all(np.diff(lam) < 0)
    ch, e = em.fit(x, lab, 2, 7, len_in, 0.0)
    _, mu, _, W, B = em.scatter(x, lab, len_in)
    assert np.allclose(ch.A @ W @ ch.A.T, np.eye(7), atol=1e-10)
    G = ch.A @ B @ ch.A.T
    assert np.allclose(G, np.diag(e), atol=1e-9 * e[0]) and np.all(np.diff(e) < 0)
    assert np.allclose(ch.m_out, ch.A @ mu)
    try:
        from scipy.linalg import eigh
    except ImportError:
        return
    assert np.allclose(eigh(B, W, eigvals_only=True)[::-1][:7], e, rtol=1e-9)
    ch0, _ = em.fit(x, None, 0, 12, len_in, 1.0)
    assert ch0.A is None and np.allclose(ch0.m_out, mu)


def test_chain_validation():
    with pytest.raises(ValueError):
        EmbeddingChain()                                       # no dimension
    with pytest.raises(ValueError):
        EmbeddingChain(np.zeros(4), A=np.zeros((3, 5)))        # m_in against A
    with pytest.raises(ValueError):
        EmbeddingChain(A=np.zeros((3, 5)), m_out=np.zeros(5))  # m_out against A
    with pytest.raises(ValueError):
        EmbeddingChain(np.zeros(4), m_out=np.zeros(3))         # no A: Dout == Din
    with pytest.raises(ValueError):
        EmbeddingChain(np.zeros(4), len_in=-1.0)
    with pytest.raises(ValueError):
        EmbeddingChain(np.zeros(4), len_out=np.inf)
    with pytest.raises(ValueError):
        EmbeddingChain(np.array([0.0, np.nan]))
    with pytest.raises(ValueError):
        EmbeddingChain(A=np.full((2, 2), np.inf))
    with pytest.raises(ValueError):
        EmbeddingChain(np.zeros(4097))
    with pytest.raises(ValueError):
        EmbeddingChain(A=np.zeros((2049, 4)))
    c = EmbeddingChain(np.zeros(5), 0.0, np.ones((3, 5)), None, 2.0)
    assert (c.din, c.dout) == (5, 3) and c.m_out is None
    assert (EmbeddingChain(dim=6).din, EmbeddingChain(dim=6).dout) == (6, 6)


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("single", [True, False])
def test_kaldi_vector_matrix_round_trip(tmp_path, binary, single):
    rng = np.random.default_rng(6)
    v, m = rng.standard_normal(7), rng.standard_normal((3, 5))
    kaldi_io.write_vector(tmp_path / "v", v, binary, single)
    kaldi_io.write_matrix(tmp_path / "m", m, binary, single)
    want_v = v.astype(np.float32).astype(np.float64) if single else v
    want_m = m.astype(np.float32).astype(np.float64) if single else m
    assert np.array_equal(kaldi_io.read_vector(tmp_path / "v"), want_v)
    assert np.array_equal(kaldi_io.read_matrix(tmp_path / "m"), want_m)
    raw = open(tmp_path / "v", "rb").read()
    if binary:
        assert raw[:5] == (b"\0BFV " if single else b"\0BDV ") and raw[5:10] == b"\x04\x07\0\0\0" and len(raw) == 10 + 7 * (4 if single else 8)


def test_from_kaldi_with_and_without_offset(tmp_path):
    rng = np.random.default_rng(7)
    mean, A, off = rng.standard_normal(6), rng.standard_normal((4, 6)), rng.standard_normal(4)
    kaldi_io.write_vector(tmp_path / "mean.vec", mean)
    kaldi_io.write_matrix(tmp_path / "t.mat", A)
    kaldi_io.write_matrix(tmp_path / "t_off.mat", np.hstack([A, off[:, None]]), binary=False)
    c = EmbeddingChain.from_kaldi(tmp_path / "mean.vec", tmp_path / "t.mat")
    assert np.array_equal(c.m_in, mean) and np.array_equal(c.A, A) and c.m_out is None and c.len_in == 0 and c.len_out == 2.0
    c = EmbeddingChain.from_kaldi(tmp_path / "mean.vec", tmp_path / "t_off.mat", normalize_length=False)
    assert np.array_equal(c.A, A) and np.array_equal(c.m_out, -off) and c.len_out == 0
    c = EmbeddingChain.from_kaldi(tmp_path / "mean.vec")
    assert c.A is None and (c.din, c.dout) == (6, 6) and c.len_out == np.sqrt(6)
    kaldi_io.write_matrix(tmp_path / "bad.mat", rng.standard_normal((4, 9)))
    with pytest.raises(ValueError):
        EmbeddingChain.from_kaldi(tmp_path / "mean.vec", tmp_path / "bad.mat")
    # x -> A x + offset (transform-vec with an offset column) is the chain's A v - m_out
    x = rng.standard_normal((3, 6))
    c = EmbeddingChain.from_kaldi(tmp_path / "mean.vec", tmp_path / "t_off.mat", normalize_length=False)
    assert np.allclose(em.apply(em.Chain(c.m_in, c.len_in, c.A, c.m_out, c.len_out), x), (x - mean) @ A.T + off)


def test_signatures_hold_the_nine_entry_points():
    want = {"plda_embed_set": 8, "plda_embed_clear": 1, "plda_embed_dims": 4, "plda_embed_get": 6, "plda_embed_plan": 6,
            "plda_embed_apply_dev": 6, "plda_embed_apply": 6, "plda_embed_fit_dev": 12, "plda_embed_fit": 11}
    for name, nargs in want.items():
        assert name in N.SIGNATURES and len(N.SIGNATURES[name][1]) == nargs, name


def test_npz_has_no_embed_keys_without_a_chain(tmp_path):
    """save() of a model without a chain writes the keys it wrote before: the five embed_* keys appear only with one."""
    from plda_amd.libplda import MPlda

    class Fake(MPlda):
        def __init__(self):
            self._meanz, self._stdvz, self._calibration, self._embedding = {}, {}, None, None

        def get_model(self):
            return dict(mean=np.zeros(3), transform=np.eye(3), psi=np.ones(3))

        def __del__(self):
            pass

    f = Fake()
    f.save(tmp_path / "m.npz")
    assert not [k for k in np.load(tmp_path / "m.npz").files if k.startswith("embed_")]
    f._embedding = EmbeddingChain(np.arange(3.0), 0.0, None, None, 1.5)
    f.save(tmp_path / "m2.npz")
    z = np.load(tmp_path / "m2.npz")
    assert sorted(k for k in z.files if k.startswith("embed_")) == ["embed_A", "embed_len_in", "embed_len_out", "embed_m_in", "embed_m_out"]
    assert z["embed_A"].size == 0 and z["embed_m_out"].size == 0 and np.array_equal(z["embed_m_in"], np.arange(3.0))
