"""GPU: the SPD inverse of the EM's E-step (Kaldi SpMatrix::Invert at ivector/plda.cc:436-447) on its own, through
plda_spd_inverse: the scalar sweep in registers (D <= 64), the block sweep on the fp64 matrix cores (D <= 256: 16
pivots per step, tiles of the triangle in MFMA accumulators) and the blocked whitening above, against
numpy.linalg.inv in the residual norm that the condition number allows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _spd(d, cond, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    lam = np.exp(np.linspace(0.0, np.log(cond), d))
    a = (q * lam) @ q.T
    return 0.5 * (a + a.T)


_SMALL = [1, 7, 16, 17, 33, 48, 64, 65, 80, 81, 96, 100, 112, 113, 127, 128, 140, 144, 150, 161, 176, 192, 200, 207, 208,
          209, 224, 240, 255, 256]


def _small_kernel(d, variant):
    """the kernel of spd_inverse_small (csrc/linalg.hip) at size d <= 256 under PLDA_SWEEP_VARIANT=variant"""
    if variant == "0" and d > 64:
        return "spd_inverse_mfma_kernel<%d,0>" % -(-d // 16)
    if variant in ("0", "2"):
        return "spd_inverse_sweep16_kernel<%d>" % -(-d // 16)
    return "spd_inverse_sweep_kernel<%d>" % -(-d // 32)


def test_small_sizes_cover_every_instantiation():
    """the size list reaches spd_inverse_sweep16_kernel<1..16> (variant 2), spd_inverse_mfma_kernel<5..16, 0> (default) and
    spd_inverse_sweep_kernel<1..8> (variant 1); each size asserts its own kernel below"""
    assert {_small_kernel(d, "2") for d in _SMALL} == {"spd_inverse_sweep16_kernel<%d>" % nb for nb in range(1, 17)}
    assert {_small_kernel(d, "0") for d in _SMALL if d > 64} == {"spd_inverse_mfma_kernel<%d,0>" % nt for nt in range(5, 17)}
    assert {_small_kernel(d, "1") for d in _SMALL} == {"spd_inverse_sweep_kernel<%d>" % nb for nb in range(1, 9)}


@pytest.mark.parametrize("variant", ["0", "2", "1"])
@pytest.mark.parametrize("d", _SMALL)
def test_small_inverse_every_block_count(monkeypatch, d, variant):
    from plda_amd import MPlda
    monkeypatch.setenv("PLDA_SWEEP_VARIANT", variant)
    eng = MPlda(0)
    for cond, seed in ((10.0, 1), (1e6, 2)):
        a = _spd(d, cond, seed + d)
        got = eng.spd_inverse(a)
        assert eng.linalg_last_kernels() == [_small_kernel(d, variant)], (d, variant, eng.linalg_last_kernels())
        assert np.array_equal(got, got.T)
        res = np.abs(got @ a - np.eye(d)).max()
        assert res < 5e-16 * cond * d + 1e-13, (d, cond, res)
        want = np.linalg.inv(a)
        assert np.abs(got - want).max() <= 1e-15 * cond * d * np.abs(want).max() + 1e-14


def test_block_sweep_agrees_with_the_scalar_sweep(monkeypatch):
    """The block form is the same elimination grouped by 16 pivots: entries agree to rounding."""
    from plda_amd import MPlda
    a = _spd(200, 1e4, 5)
    monkeypatch.setenv("PLDA_SWEEP_VARIANT", "0")
    x0 = MPlda(0).spd_inverse(a)
    monkeypatch.setenv("PLDA_SWEEP_VARIANT", "2")
    x2 = MPlda(0).spd_inverse(a)
    assert np.abs(x0 - x2).max() <= 1e-12 * np.abs(x2).max()


@pytest.mark.parametrize("d", [257, 300, 512])
def test_blocked_inverse(d):
    from plda_amd import MPlda
    a = _spd(d, 1e3, d)
    got = MPlda(0).spd_inverse(a)
    assert np.abs(got @ a - np.eye(d)).max() < 1e-10


def _leaves(n):
    """the diagonal blocks that whiten_blocked (csrc/linalg.hip) factors in one kernel: n1 = round_up(ceil(n / 2), 32)"""
    if n <= 256:
        return [n]
    n1 = -(-(-(-n // 2)) // 32) * 32
    return _leaves(n1) + _leaves(n - n1)


# 420 is not in the list the sizes were drawn up from: it is the one that splits into a leaf of 13 tile rows (224 + 196)
_BLOCKED = [(n, cond) for n in (257, 272, 273, 288, 289, 320, 321, 352, 353, 416, 420, 480, 512, 513, 576, 577, 1024, 1025)
            for cond in (10.0, 1e6)] + [(2048, 10.0)]


def test_blocked_sizes_cover_every_leaf_kernel():
    """the leaves of the sizes below are whitened by spd_inverse_mfma_kernel<7..16, 1>, each at least once"""
    assert {-(-m // 16) for n, _ in _BLOCKED for m in _leaves(n)} == set(range(7, 17))


@pytest.mark.parametrize("d,cond", _BLOCKED)
def test_blocked_inverse_split_rule_and_recursion(d, cond):
    """The blocked path (D > 256: T = whiten(A) by block elimination, A^-1 = T^T T) at the sizes where the split
    n1 = round_up(ceil(n / 2), 32) changes the leaves' tile counts, one and two levels of recursion and the largest size,
    held to the bound of the small sizes; the leaves are asserted from the kernels the library reports."""
    from plda_amd import MPlda
    eng = MPlda(0)
    a = _spd(d, cond, 3 + d)
    got = eng.spd_inverse(a)
    ran = eng.linalg_last_kernels()
    assert {k for k in ran if k.startswith("spd_inverse")} == {"spd_inverse_mfma_kernel<%d,1>" % -(-m // 16) for m in _leaves(d)}, (d, ran)
    assert np.array_equal(got, got.T)
    res = np.abs(got @ a - np.eye(d)).max()
    want = np.linalg.inv(a)
    print("blocked inverse d=%d cond=%g: |XA - I| %.3e (bound %.3e; numpy.linalg.inv %.3e), |X - inv| %.3e (bound %.3e)" % (
        d, cond, res, 5e-16 * cond * d + 1e-13, np.abs(want @ a - np.eye(d)).max(), np.abs(got - want).max(),
        1e-15 * cond * d * np.abs(want).max() + 1e-14))
    assert res < 5e-16 * cond * d + 1e-13, (d, cond, res)
    assert np.abs(got - want).max() <= 1e-15 * cond * d * np.abs(want).max() + 1e-14


def test_not_positive_definite_is_an_error():
    from plda_amd import MPlda
    a = _spd(100, 10.0, 3)
    a[50, 50] = -1.0
    with pytest.raises(RuntimeError):
        MPlda(0).spd_inverse(a)
