"""CPU: the conditions that make the front-end's GPU edge tests mean something (tests/frontend_model.py).

The offset-variance cases must (a) have a reference, fp64 np.var, that is itself good to well under the GPU tolerance
of 1e-10, measured against the definition in extended precision, and (b) break the one-pass formula the pooling
kernels used by far more than that tolerance -- otherwise a kernel that still used it would pass.  The 64-ary search
model must agree with the definition on every offset table the HTK cases decode."""
import numpy as np
import pytest

import frontend_model as fm


def test_extended_precision_is_extended():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


@pytest.mark.parametrize("name,d,dtype", fm.var_cases())
def test_reference_variance_is_accurate(name, d, dtype):
    x, l2norm = fm.var_case(name, d, dtype)
    ref = np.var(fm.normalised(x, l2norm), axis=0)
    ext = fm.var_extended(x, l2norm)
    assert (ext > 0).all()
    err = fm.rel_err(ref, ext)
    print("%s d=%d %s: np.var %.2e" % (name, d, dtype, err))
    assert err <= 1e-11


@pytest.mark.parametrize("name,d,dtype", fm.var_cases())
def test_one_pass_loses_offset_cases_and_shift_keeps_them(name, d, dtype):
    x, l2norm = fm.var_case(name, d, dtype)
    y = fm.normalised(x, l2norm)
    ext = fm.var_extended(x, l2norm)
    old, new = fm.rel_err(fm.var_one_pass(y), ext), fm.rel_err(fm.var_shifted(y), ext)
    print("%s d=%d %s: one-pass %.2e, shifted %.2e" % (name, d, dtype, old, new))
    if fm.VAR_CASES[name][3]:
        assert old > 1e-8                  # 100 x the GPU tolerance
    else:
        assert old <= 1e-11                # the control: nothing to lose
    assert new <= 1e-11


def test_case_shapes_and_dtypes():
    for name, d, dtype in fm.var_cases():
        x, _ = fm.var_case(name, d, dtype)
        assert x.shape == (fm.VAR_CASES[name][2], d) and x.dtype == np.dtype(dtype) and np.isfinite(x).all()
        again, _ = fm.var_case(name, d, dtype)
        assert np.array_equal(x, again)
    x, l2norm = fm.var_case("dominant_column", 64, np.float32)
    assert l2norm and (x[:, 0] == 1e3).all()


@pytest.mark.parametrize("name", sorted(fm.search_tables()))
def test_search_model_finds_the_last_file_at_or_before(name):
    counts = fm.search_tables()[name]
    off = fm.offsets_of(counts)
    T = int(off[-1])
    # every chunk start of the chunk sizes the cases use, and every frame of a short batch
    starts = set(range(T)) if T <= 3000 else set()
    for fr in (1, 4, 204, 210, 256):
        starts.update(range(0, T, fr))
    for t0 in sorted(starts):
        u = fm.search_model(off, t0)
        assert u == fm.search_expected(off, t0), (name, t0)
        assert off[u] <= t0 and (off[u + 1:-1] > t0).all()


def test_search_model_on_random_tables():
    rng = np.random.default_rng(1)
    for _ in range(200):
        u = int(rng.integers(1, 9000))
        counts = rng.integers(0, 4, u) * (rng.random(u) < rng.random())
        if counts.sum() == 0:
            counts[int(rng.integers(0, u))] = 1
        off = fm.offsets_of(counts)
        for t0 in rng.integers(0, off[-1], 20):
            assert fm.search_model(off, int(t0)) == fm.search_expected(off, int(t0))


def test_chunk_frames():
    assert [fm.chunk_frames(w, f) for w, f in ((13, 0), (13, 1), (39, 2), (1, 0), (40, 0), (8, 1), (700, 6), (2048, 0))] == \
        [256, 210, 42, 256, 204, 256, 1, 4]
