"""GPU: the d-vector pooling kernels (csrc/frontend.hip) through the device entry plda_dvector_pool_dev, at every
dispatch class and at the edges where they can go wrong, against oracle.plda_oracle_np.dvector_pool on the fp64 cast.

Every call is set up the way tests/test_gpu_guard_bands.py sets its calls up: frames and offsets are views inside
NaN-filled buffers, the utterances own only the middle of the frames (offsets[0] > 0, offsets[U] < T), the output
sits between guards that must survive while every element is written, and the result must be bit-identical when the
neighbours hold zero instead.

Tolerances: mean and max within 1e-12 * max(max |ref|, 1) for float32 and float64 frames alike (a float32 frame
converts exactly and the accumulation is fp64); var per column within 1e-10 of that column's reference variance:
the shifted one-pass form is bounded by about n eps (1 + ((y0 - mean) / std)^2), 2e-12 at n = 1000, the reference's own
error is below 1e-11 (tests/test_frontend_model.py), and the unshifted form misses by 1e-8 to 1e+3 on the offset
cases."""
import functools

import numpy as np
import pytest

import frontend_model as fm
from test_gpu_guard_bands import PAYLOAD, _Output, _both, _input

pytestmark = pytest.mark.gpu

METHODS = {"mean": 0, "max": 1, "var": 2}
LEAD, TRAIL = 3, 5                       # unowned frames before and after the utterances
VEC_DIMS = (16, 32, 64, 128, 256)        # float32 and 16-byte aligned: dvector_pool_vec4_kernel<G>, G = D / 4
SCALAR_DIMS = (1, 3, 63, 64, 65, 255, 257, 511, 513, 1023, 1024)
# straddles 4 * FPW * UNR = 1024 / G frames per block iteration of every G and the scalar kernel's stride of 4;
# shuffled, an empty utterance first, in the middle and last
LENGTHS = (0, 257, 4, 1025, 16, 63, 1, 513, 0, 65, 255, 2, 17, 511, 5, 64, 3, 256, 15, 0)
assert sorted(set(LENGTHS)) == [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 513, 1025]


@pytest.fixture(scope="module")
def eng():
    from plda_amd import MPlda
    yield MPlda(0)
    _class_dev.cache_clear()             # the device buffers the dispatch-class tests share


class _Frames:
    """Owned frames [n, D] on the device with LEAD / TRAIL unowned frames around them, inside a guarded buffer whose
    unowned parts hold NaN (or zero); the view starts `shift` bytes past a 16-byte boundary."""

    def __init__(self, x, nan, shift=0):
        x = np.ascontiguousarray(x)
        n, d = x.shape
        k = shift // x.itemsize
        assert k * x.itemsize == shift
        fill = np.nan if nan else 0.0
        flat = np.concatenate([np.full(k + LEAD * d, fill, x.dtype), x.ravel(), np.full(TRAIL * d, fill, x.dtype)])
        self.buf, body = _input(flat, nan)
        self.view = body.reshape(-1)[k:].view(LEAD + n + TRAIL, d)
        assert self.view.data_ptr() % 16 == shift
        self.T, self.D, self.dtype = LEAD + n + TRAIL, d, 0 if x.dtype == np.float32 else 1


def _pool_dev(eng, fr, lens, method, l2norm, nan):
    """One call of the device entry on prepared frames; the checked output as a host array."""
    import torch
    off = LEAD + fm.offsets_of(lens)
    assert off[-1] == fr.T - TRAIL
    _, doff = _input(off, nan)
    out = _Output(len(lens), fr.D, torch.float64)
    torch.cuda.synchronize()
    eng._ck(eng._lib.plda_dvector_pool_dev(eng._h, fr.view.data_ptr(), fr.dtype, fr.T, fr.D, doff.data_ptr(), len(lens),
                                           METHODS[method], int(l2norm), out.ptr()))
    eng.synchronize()
    return out.check("%s l2norm=%d D=%d" % (method, l2norm, fr.D))


def _reference(x, lens, method, l2norm):
    """The oracle per utterance on the fp64 cast; an empty utterance is a NaN row (np.mean of nothing)."""
    from oracle import plda_oracle_np as onp
    x = np.asarray(x, np.float64)
    off = fm.offsets_of(lens)
    ref = np.full((len(lens), x.shape[1]), np.nan)
    with np.errstate(all="ignore"):
        for u in range(len(lens)):
            if lens[u]:
                ref[u] = onp.dvector_pool(x, off[u:u + 2], method, l2norm)[0]
    return ref


def _close(got, ref, method, what=""):
    """NaN and Inf where the reference has them, bit for bit; the tolerance of the module docstring elsewhere."""
    assert got.shape == ref.shape and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), what
    fin = np.isfinite(ref)
    if not fin.any():
        return
    err = np.abs(got[fin] - ref[fin])
    if method == "var":
        bound = 1e-10 * ref[fin]
    else:
        bound = 1e-12 * max(np.abs(ref[fin]).max(), 1.0)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%s %s: worst error / bound = %.3g" % (what, method, worst))
    assert (err <= bound).all(), "%s %s: error is %.3g x the bound" % (what, method, worst)


# ---------------------------------------------------------------------------------------- dispatch classes
@functools.lru_cache(maxsize=None)
def _class_host(d, dtype):
    rng = np.random.default_rng([7, d])
    return (3.0 * rng.standard_normal((sum(LENGTHS), d)) + 0.5).astype(dtype)


@functools.lru_cache(maxsize=None)
def _class_dev(d, dtype, nan, shift):
    return _Frames(_class_host(d, dtype), nan, shift)


@functools.lru_cache(maxsize=None)
def _class_ref(d, dtype, method, l2norm):
    return _reference(_class_host(d, dtype), LENGTHS, method, l2norm)


def _class_case(eng, d, dtype, method, l2norm, shift=0):
    a = _both(lambda nan: dict(p=_pool_dev(eng, _class_dev(d, dtype, nan, shift), LENGTHS, method, l2norm, nan)))["p"]
    empty = np.asarray(LENGTHS) == 0
    assert np.isnan(a[empty]).all() and not np.isnan(a[~empty]).any()     # an empty utterance is a NaN row in every class
    _close(a, _class_ref(d, dtype, method, l2norm), method, "D=%d %s shift=%d l2norm=%d" % (d, dtype, shift, l2norm))
    return a


@pytest.mark.parametrize("l2norm", [True, False])
@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("d", VEC_DIMS)
def test_vec4_classes_and_their_misaligned_fallback(eng, d, method, l2norm):
    """float32 at D = 4 G: the vec4 kernel when the frames are 16-byte aligned, the scalar kernel when the pointer is
    4 or 8 bytes past that; all three agree with the oracle and, at the same tolerance, with each other."""
    aligned = _class_case(eng, d, "float32", method, l2norm)
    for shift in (4, 8):
        got = _class_case(eng, d, "float32", method, l2norm, shift)
        _close(got, aligned, method, "D=%d shift=%d against the aligned call" % (d, shift))


@pytest.mark.parametrize("l2norm", [True, False])
@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("d", VEC_DIMS + SCALAR_DIMS)
def test_float64_classes(eng, d, method, l2norm):
    _class_case(eng, d, "float64", method, l2norm)


@pytest.mark.parametrize("l2norm", [True, False])
@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("d", SCALAR_DIMS)
def test_float32_scalar_classes(eng, d, method, l2norm):
    _class_case(eng, d, "float32", method, l2norm)


# ---------------------------------------------------------------------------------------- offset variance
@pytest.mark.parametrize("name,d,dtype", fm.var_cases())
def test_variance_of_offset_frames(eng, name, d, dtype):
    """The cases of tests/frontend_model.py, between two ordinary utterances so that the shift is not frame 0."""
    x, l2norm = fm.var_case(name, d, dtype)
    rng = np.random.default_rng(5)
    lens = [17, len(x), 5]
    frames = np.concatenate([(3 * rng.standard_normal((17, d))).astype(dtype), x, (3 * rng.standard_normal((5, d))).astype(dtype)])
    a = _both(lambda nan: dict(p=_pool_dev(eng, _Frames(frames, nan), lens, "var", l2norm, nan)))["p"]
    ref = _reference(frames, lens, "var", l2norm)
    print("%s D=%d %s: worst relative error per column %.3g" % (name, d, dtype, fm.rel_err(a[1], ref[1])))
    _close(a, ref, "var", "%s D=%d %s" % (name, d, dtype))


# ---------------------------------------------------------------------------------------- non-finite values
NONFINITE_CLASSES = [(16, "float32"), (64, "float32"), (256, "float32"), (10, "float32"), (16, "float64"), (300, "float64")]
NAN_FRAMES = (0, 1, 17, 64, 130, 200, 299)       # every wave; in the vec4 kernels frame groups other than the first


def _special(d, dtype, edit):
    """Three utterances of 9, 300 and 4 frames; `edit` changes the middle one in place.  -> frames, lens"""
    rng = np.random.default_rng([11, d])
    lens = [9, 300, 4]
    x = (rng.standard_normal((sum(lens), d)) + 0.25).astype(dtype)
    edit(x[9:309])
    return x, lens


def _special_case(eng, x, lens, method, l2norm):
    a = _both(lambda nan: dict(p=_pool_dev(eng, _Frames(x, nan), lens, method, l2norm, nan)))["p"]
    _close(a, _reference(x, lens, method, l2norm), method)
    assert np.isfinite(a[[0, 2]]).all()              # the neighbours of the special utterance are untouched by it
    return a[1]


@pytest.mark.parametrize("j", NAN_FRAMES)
@pytest.mark.parametrize("d,dtype", NONFINITE_CLASSES)
def test_one_nan_element(eng, d, dtype, j):
    col = min(5, d - 1)

    def edit(u):
        u[j, col] = np.nan
    x, lens = _special(d, dtype, edit)
    for method in METHODS:
        row = _special_case(eng, x, lens, method, False)
        assert np.isnan(row[col]) and np.isfinite(np.delete(row, col)).all(), (method, "only that column is NaN")
        row = _special_case(eng, x, lens, method, True)
        assert np.isnan(row).all(), (method, "the frame's norm is NaN, so is the whole row")


@pytest.mark.parametrize("d,dtype", NONFINITE_CLASSES)
def test_infinities_and_zero_frame(eng, d, dtype):
    col = d - 1

    def plus_inf(u):
        u[130, col] = np.inf
    x, lens = _special(d, dtype, plus_inf)
    assert _special_case(eng, x, lens, "max", False)[col] == np.inf
    assert _special_case(eng, x, lens, "mean", False)[col] == np.inf
    row = _special_case(eng, x, lens, "var", False)
    assert np.isnan(row[col]) and np.isfinite(np.delete(row, col)).all()

    def minus_inf_column(u):
        u[:, col] = -np.inf
    x, lens = _special(d, dtype, minus_inf_column)
    row = _special_case(eng, x, lens, "max", False)
    assert row[col] == -np.inf and np.isfinite(np.delete(row, col)).all()
    assert _special_case(eng, x, lens, "mean", False)[col] == -np.inf

    def zero_frame(u):
        u[200] = 0.0
    x, lens = _special(d, dtype, zero_frame)
    for method in METHODS:
        assert np.isnan(_special_case(eng, x, lens, method, True)).all(), (method, "0 / 0 in one frame")
        assert np.isfinite(_special_case(eng, x, lens, method, False)).all()


# ---------------------------------------------------------------------------------------- many utterances
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_seventy_thousand_one_frame_utterances(eng, dtype):
    """A grid above 65 535 workgroups (vec4 kernel for float32, scalar for float64).  One frame per utterance: without
    l2norm mean and max are that frame and the variance is 0, exactly; with it the variance is still exactly 0 and mean
    and max are one and the same value, the frame over its norm (to the tolerance: the order of the norm's sum is the
    kernel's own)."""
    U, d = 70000, 16
    x = (np.random.default_rng(70).standard_normal((U, d)) + 2.0).astype(dtype)
    lens = np.ones(U, np.int64)
    got = {}
    for l2norm in (False, True):
        for method in METHODS:
            got[method, l2norm] = _both(lambda nan: dict(p=_pool_dev(eng, _Frames(x, nan), lens, method, l2norm, nan)))["p"]
        assert not got["var", l2norm].any()
        assert np.array_equal(got["mean", l2norm], got["max", l2norm])
    assert np.array_equal(got["mean", False], x.astype(np.float64))
    x64 = x.astype(np.float64)
    _close(got["mean", True], x64 / np.linalg.norm(x64, axis=1)[:, None], "mean")


# ---------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_handle_usable(eng):
    import torch
    from plda_amd import _native as N
    lens = [3, 0, 7]
    x = np.random.default_rng(1).standard_normal((10, 16)).astype(np.float32)
    fr = _Frames(x, True)
    _, doff = _input(LEAD + fm.offsets_of(lens), True)
    out = _Output(3, 16, torch.float64)
    fp, op, dp = fr.view.data_ptr(), doff.data_ptr(), out.ptr()
    call = eng._lib.plda_dvector_pool_dev
    bad = dict(D1025=(fp, 0, fr.T, 1025, op, 3, 0, 1, dp), method3=(fp, 0, fr.T, 16, op, 3, 3, 1, dp),
               dtype2=(fp, 2, fr.T, 16, op, 3, 0, 1, dp), no_frames=(None, 0, fr.T, 16, op, 3, 0, 1, dp),
               no_offsets=(fp, 0, fr.T, 16, None, 3, 0, 1, dp), no_output=(fp, 0, fr.T, 16, op, 3, 0, 1, None))
    for what, args in bad.items():
        assert call(eng._h, *args) == N.PLDA_E_INVAL, what
        assert "dvector_pool" in N.last_error(eng._h), what
    assert call(eng._h, fp, 0, fr.T, 16, op, 0, 0, 1, dp) == N.PLDA_OK            # U = 0: nothing to do
    assert call(eng._h, None, 0, 0, 16, None, 0, 0, 1, None) == N.PLDA_OK
    eng.synchronize()
    assert bool((out.words == PAYLOAD).all()), "a refused or empty call wrote to the output"
    got = _pool_dev(eng, fr, lens, "mean", True, True)                               # the handle still works
    _close(got, _reference(x, lens, "mean", True), "mean")
