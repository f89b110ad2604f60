"""GPU: PLDA.fit and transform on rows with a common offset (tests/fit_model.py states what they must compute).

The statistics pass (csrc/fit.hip:fit_stats_device) formed its offset scatter as Kaldi's AddSamples does, as the difference of two
uncentred sums  X^T diag(1 / n_label) X - M^T M,  and so did both oracles: the suite compared one cancellation with another on
uniform [0, 1) rows, where it cannot show.  Here the rows lie on the grid 2^-20 and are shifted by exact powers of two, so the
expected statistics and model follow from the oracle's fit of the UNSHIFTED rows by identities, and the scatter is held to an
extended-precision product of class-centred rows -- in every dispatch class of the product, both label groupings, whole fits in
every EM form, degenerate classes, sharded by speaker, on reused buffers.

Measured on an MI355X with the library as it was before it centred its rows (ranges over the shapes below; relative to max |S|,
max |W|, max psi), beside what tests/test_fit_model.py computes for the same formula in NumPy on the same rows:

    shift     scatter, device       scatter, NumPy       W, device            W, NumPy             psi, device          psi, NumPy
     1024     6.2e-9 .. 3.7e-8      9.0e-9 .. 1.4e-8     6.3e-9 .. 1.3e-8     8.4e-9 .. 1.4e-8     2.9e-9 .. 1.2e-8     1.7e-9 .. 9.7e-9
     8192     3.7e-7 .. 2.9e-6      3.3e-7 .. 9.9e-7     3.5e-7 .. 7.6e-7     3.1e-7 .. 9.9e-7     2.4e-7 .. 5.6e-7     4.4e-7 .. 7.1e-7
   131072     9.6e-5 .. 6.9e-4      1.3e-4 .. 2.5e-4     9.5e-5 .. 2.0e-4     1.2e-4 .. 2.5e-4     4.3e-5 .. 1.2e-4     8.1e-6 .. 1.1e-4

against 1e-10 and 1e-9 allowed (the upper ends of the device's scatter are the weighted GEMM at D = 209 and 513); every case at a
shift of 1024 or more failed, every case at shift 0 met its tolerances.  All-singleton classes at 8192 left up to 5e-6 of
rounding noise where the scatter is exactly zero and 3e-11 is allowed.  The transform was inside its bound before and after
(0.004 .. 0.03 of it).  With class-centred rows the scatter is within 3.2e-15 at every shift and shape, W, B and psi within
4e-11 (131072: the rounding of class means of that size), and the degenerate cases give exact zeros.
"""
import functools

import numpy as np
import pytest

import fit_model as M

pytestmark = pytest.mark.gpu

SCATTER_TOL = 1e-10          # tests/test_gpu_fit.py:test_fit_matches_oracle
MODEL_TOL = 1e-9
STATS_SHIFT = 8192.0         # the one shift of the arms, the degenerate classes, the shards and the reuse


@functools.lru_cache(maxsize=None)
def _data(n, d, k, singles=0, const_cols=()):
    return M.grid_data(n + d + k, n, d, k, singles=singles, const_cols=const_cols)


@functools.lru_cache(maxsize=None)
def _scatter_ref(n, d, k, singles=0, const_cols=()):
    x, y = _data(n, d, k, singles, const_cols)
    return M.scatter_longdouble(x, y)


def _engine(monkeypatch, **env):
    """A handle created under the given PLDA_* knobs (they are read when a handle is created)."""
    from plda_amd import MPlda
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    eng = MPlda(0)
    for key in env:
        monkeypatch.delenv(key)
    return eng


def _stats(eng, x, y, k):
    """plda_fit_stats_dev + plda_fit_get_stats_dev -> (means, counts, scatter) on the host."""
    import torch
    dev = torch.device("cuda", 0)
    n, d = x.shape
    dx = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    dy = torch.from_numpy(y.astype(np.int64)).to(dev)
    means = torch.empty((k, d), dtype=torch.float64, device=dev)
    counts = torch.empty((k,), dtype=torch.int64, device=dev)
    scatter = torch.empty((d, d), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    eng.fit_stats_dev(dx.data_ptr(), n, d, dy.data_ptr(), k)
    eng.fit_get_stats_dev(means.data_ptr(), counts.data_ptr(), scatter.data_ptr())
    eng.synchronize()
    return means.cpu().numpy(), counts.cpu().numpy(), scatter.cpu().numpy()


def _check_stats(got, x, y, c, want_scatter, what="", symmetric=True):
    """Counts exactly; the class means inside fit_model.mean_bound (n_k u max|x|, derived there) of the extended-precision means
    of the SHIFTED rows; the scatter within 1e-10 max|S| of the extended-precision product of class-centred rows, and exactly
    symmetric where a SYRK kernel formed it (they give both mirror elements the same sum; the weighted general GEMM of odd D
    above 208 and of D above 512 rounds (w x_i) x_j and (w x_j) x_i apart, before this change as after it)."""
    means, counts, scatter = got
    xs = x + c
    want_counts = np.bincount(y.astype(np.int64))
    assert np.array_equal(counts, want_counts)
    e_m = float((np.abs(means - M.means_longdouble(xs, y)) / M.mean_bound(want_counts, np.abs(xs).max())).max())
    e_s = float(np.abs(scatter - want_scatter).max() / np.abs(want_scatter).max())
    print("%s shift %6d: scatter off by %.3g of max|S|, means by %.3g of their bound" % (what, int(c), e_s, e_m))
    assert e_m <= 1.0, e_m
    assert e_s <= SCATTER_TOL, e_s
    assert not symmetric or np.array_equal(scatter, scatter.T)


def _scatter_kernels(eng):
    """The kernels of the scatter product on a handle that has run nothing else (template arguments dropped)."""
    return [k.split("<")[0] for k in eng.linalg_last_kernels()]


# ------------------------------------------------------------------------------------------- (a) the statistics pass, every dispatch class
_PATH = {6: "syrk_tri_kernel", 33: "syrk_tri_kernel", 208: "syrk_tri_kernel", 209: "gemm_f64_kernel", 210: "syrk_blk_kernel",
         300: "syrk_blk_kernel", 513: "gemm_f64_kernel", 211: "syrk_lower_kernel"}


@pytest.mark.parametrize("c", M.SHIFTS)
@pytest.mark.parametrize("d,n,k", M.STAT_SHAPES + [(211, 2100, 11)])
def test_statistics_pass_on_offset_rows(d, n, k, c):
    """D = 208 is the last size of the triangle kernel; the block kernel takes EVEN D from 210 to 512, so D = 209 and D = 513
    run the plain GEMM with row weights -- which hands 2048 rows or more to the super-tile SYRK (D = 211, N = 2100).  N and K
    are no multiples of the 16-row stage."""
    from plda_amd import MPlda
    x, y = _data(n, d, k)
    M.assert_exact_shift(x, c)
    eng = MPlda(0)
    got = _stats(eng, x + c, y, k)
    kernels = _scatter_kernels(eng)
    _check_stats(got, x, y, c, _scatter_ref(n, d, k), "D = %d (%s)" % (d, " ".join(kernels)), _PATH[d] != "gemm_f64_kernel")
    assert kernels[0] == _PATH[d] and all(name.startswith(("syrk_tri_reduce", "syrk_reduce", _PATH[d])) for name in kernels), kernels


@pytest.mark.parametrize("variant,d,path", [("0", 33, "syrk_tri_kernel"), ("6", 33, "syrk_tri_kernel"), ("3", 33, "gemm_f64_kernel"),
                                            ("1", 33, "gemm_f64_kernel"), ("0", 300, "syrk_blk_kernel"), ("6", 300, "gemm_f64_kernel"),
                                            ("3", 300, "gemm_f64_kernel"), ("1", 300, "gemm_f64_kernel")])
def test_statistics_pass_in_every_arm_of_the_product(monkeypatch, variant, d, path):
    """PLDA_GEMM64_VARIANT: syrk_pair_f64 takes the triangle kernel for 0 and 6 (D <= 208) and the block kernel only for 0;
    every other value -- 3, and 1 with the GEMM's own 64 x 64 tiles -- is the weighted GEMM."""
    dd, n, k = next(s for s in M.STAT_SHAPES if s[0] == d)
    x, y = _data(n, d, k)
    eng = _engine(monkeypatch, PLDA_GEMM64_VARIANT=variant)
    got = _stats(eng, x + STATS_SHIFT, y, k)
    kernels = _scatter_kernels(eng)
    _check_stats(got, x, y, STATS_SHIFT, _scatter_ref(n, d, k), "variant %s D = %d (%s)" % (variant, d, " ".join(kernels)),
                 path != "gemm_f64_kernel")
    assert kernels[0] == path and all(name.startswith(("syrk_tri_reduce", path)) for name in kernels), kernels


@pytest.mark.parametrize("d", [33, 300])
def test_statistics_pass_under_both_label_groupings(monkeypatch, d):
    """Grouping by counting (the default at these K) and by the radix sort (PLDA_SORT_VARIANT=1, as
    tests/test_gpu_fit.py:test_grouping_by_counting_is_the_radix_sort forces it): the same statistics, bit for bit."""
    dd, n, k = next(s for s in M.STAT_SHAPES if s[0] == d)
    x, y = _data(n, d, k)
    res = []
    for variant in ("0", "1"):
        got = _stats(_engine(monkeypatch, PLDA_SORT_VARIANT=variant), x + STATS_SHIFT, y, k)
        _check_stats(got, x, y, STATS_SHIFT, _scatter_ref(n, d, k), "sort %s D = %d" % (variant, d))
        res.append(got)
    for a, b in zip(*res):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------- (b) whole fits through the identities
@functools.lru_cache(maxsize=None)
def _fit_ref(n, d, k, iters, singles=0):
    from oracle import binding
    binding.build()
    x, y = _data(n, d, k, singles)
    return binding.fit(x, y, iters), binding.stats(x, y)


def _check_fit(eng, x, y, c, ref, st, what=""):
    """The assertions of tests/test_gpu_fit.py:test_fit_matches_oracle at its tolerances, against the oracle's fit of the
    UNSHIFTED rows carried across the shift (fit_model.expected_fit); the class means and the model mean under their a-priori
    bounds, offset + T mean relative to |T| |mean| as tests/test_gpu_adapt.py has it."""
    d = x.shape[1]
    xs = x + c
    xmax = np.abs(xs).max()
    it = eng.fit_internals()
    g = eng.get_model()
    T, psi = g["transform"], g["psi"]
    rT, rpsi = ref["transform"], ref["psi"]
    err = dict(scatter=M.rel(it["scatter"], st["scatter"]), W=M.rel(it["W"], ref["W"]), B=M.rel(it["B"], ref["B"]),
               psi=float(np.abs(psi - rpsi).max() / max(rpsi.max(), 1e-12)), TtT=M.rel(T.T @ T, rT.T @ rT),
               TtPsiT=M.rel(T.T @ np.diag(psi) @ T, rT.T @ np.diag(rpsi) @ rT),
               means=float((np.abs(it["means"] - M.means_longdouble(xs, y)) / M.mean_bound(st["counts"], xmax)).max()),
               sum=M.rel(it["sum"], st["sum"] + c * st["class_weight"]),
               mean=float(np.abs(g["mean"] - (ref["mean"] + c)).max() / M.model_mean_bound(st["counts"], xmax)))
    print("%s shift %6d: %s" % (what, int(c), "  ".join("%s %.3g" % kv for kv in err.items())))
    np.testing.assert_array_equal(it["counts"], st["counts"])
    assert err["means"] <= 1.0 and err["sum"] < 1e-12 and err["mean"] <= 1.0, err
    assert err["scatter"] < SCATTER_TOL, err
    assert err["W"] < MODEL_TOL and err["B"] < MODEL_TOL, err
    assert (np.diff(psi) <= 0).all() and (psi >= 0).all()
    assert err["psi"] <= MODEL_TOL and err["TtT"] < MODEL_TOL and err["TtPsiT"] < MODEL_TOL, err
    assert np.abs(T @ it["W"] @ T.T - np.eye(d)).max() < 1e-9
    assert np.abs(T @ it["B"] @ T.T - np.diag(psi)).max() < 1e-9 * max(1.0, psi.max())
    assert np.abs(g["offset"] + T @ g["mean"]).max() <= 1e-12 * (np.abs(T) @ np.abs(g["mean"])).max()


_FITS = [(n, d, k, form, 10) for (n, d, k) in M.FIT_SHAPES for form in ("0", "4")] + [(1500, 210, 12, "3", 4), (1500, 210, 12, "4", 4)]


@pytest.mark.parametrize("c", M.SHIFTS)
@pytest.mark.parametrize("n,d,k,form,iters", _FITS)
def test_fit_on_offset_rows(monkeypatch, n, d, k, form, iters, c):
    x, y = _data(n, d, k)
    M.assert_exact_shift(x, c)
    ref, st = _fit_ref(n, d, k, iters)
    eng = _engine(monkeypatch, PLDA_EM_VARIANT=form)
    assert eng.fit(x + c, y, iters) is None
    _check_fit(eng, x, y, c, ref, st, "%d x %d form %s" % (n, d, form))


# -------------------------------------------------------------------------------------------------------------------- (c) degenerate classes
@pytest.mark.parametrize("d,n", [(33, 70), (210, 50), (513, 40)])
def test_scatter_of_singleton_classes_is_zero(d, n):
    """Every class has ONE row: each row is its class mean and the offset scatter is exactly zero.  The difference of uncentred
    sums left rounding noise of order u c^2 (3e-9 at c = 8192, where the rows' total variance is 0.3)."""
    from plda_amd import MPlda
    x, y = _data(n, d, n, singles=n)
    means, counts, scatter = _stats(MPlda(0), x + STATS_SHIFT, y, n)
    assert (counts == 1).all() and np.array_equal(means, (x + STATS_SHIFT)[np.argsort(y)])
    print("D = %d: max |S| = %.3g" % (d, np.abs(scatter).max()))
    assert np.abs(scatter).max() <= SCATTER_TOL * M.total_scale(x)


def test_scatter_of_a_feature_constant_within_every_class():
    """Columns 2 and 17 hold one value per class: their rows and columns of the offset scatter vanish (to the class means' own
    rounding, far below 1e-10 of the total variance), the rest is the extended-precision scatter."""
    from plda_amd import MPlda
    n, d, k, cols = 1200, 33, 40, (2, 17)
    x, y = _data(n, d, k, 0, cols)
    got = _stats(MPlda(0), x + STATS_SHIFT, y, k)
    _check_stats(got, x, y, STATS_SHIFT, _scatter_ref(n, d, k, 0, cols), "constant columns")
    s = got[2]
    worst = max(np.abs(s[list(cols), :]).max(), np.abs(s[:, list(cols)]).max())
    print("constant columns: max |S[j, :]| = %.3g" % worst)
    assert worst <= SCATTER_TOL * M.total_scale(x)


@pytest.mark.parametrize("c", M.SHIFTS)
def test_fit_with_singleton_classes_mixed_in(monkeypatch, c):
    n, d, k, singles = 400, 33, 30, 6
    x, y = _data(n, d, k, singles)
    ref, st = _fit_ref(n, d, k, 10, singles)
    assert (st["counts"][:singles] == 1).all()
    eng = _engine(monkeypatch, PLDA_EM_VARIANT="0")
    eng.fit(x + c, y, 10)
    _check_fit(eng, x, y, c, ref, st, "singletons mixed in")


# ----------------------------------------------------------------------------------------------------------------- (d) sharded by speaker
@pytest.mark.parametrize("world", [2, 3])
def test_fit_sharded_by_speaker_on_offset_rows(world):
    """tests/test_gpu_fit.py:test_fit_sharded_by_speaker_matches_single_fit on rows shifted by 8192: every shard centres its own
    classes, so the merged record (means, counts, summed scatter) is the single handle's, and the model the unshifted oracle's."""
    import torch
    from plda_amd import MPlda
    from plda_amd.sharding import speaker_shard
    n, d, k, iters = 2600, 48, 37, 6
    x, y = _data(n, d, k)
    xs = x + STATS_SHIFT
    dev = torch.device("cuda:0")
    dx = torch.from_numpy(xs).to(dev)
    ty = torch.from_numpy(y.astype(np.int64))
    eng = MPlda(0)
    means, counts, scatter = [], [], torch.zeros((d, d), dtype=torch.float64, device=dev)
    for r in range(world):
        mask = speaker_shard(ty, world, r)
        _, dense = torch.unique(ty[mask], sorted=True, return_inverse=True)
        kk = int(dense.max()) + 1
        X = dx[mask.to(dev)].contiguous()
        lab = dense.to(torch.int64).to(dev).contiguous()
        m_ = torch.empty((kk, d), dtype=torch.float64, device=dev)
        c_ = torch.empty((kk,), dtype=torch.int64, device=dev)
        s_ = torch.empty((d, d), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        eng.fit_stats_dev(X.data_ptr(), X.shape[0], d, lab.data_ptr(), kk)
        eng.fit_get_stats_dev(m_.data_ptr(), c_.data_ptr(), s_.data_ptr())
        eng.synchronize()
        means.append(m_); counts.append(c_); scatter += s_
    means, counts = torch.cat(means).contiguous(), torch.cat(counts).contiguous()
    assert means.shape[0] == k and int(counts.sum()) == n
    torch.cuda.synchronize()
    # the merged record against the yardsticks: the shards' classes in shard order
    order = np.concatenate([np.unique(y[speaker_shard(ty, world, r).numpy()]) for r in range(world)]).astype(np.int64)
    want_counts = np.bincount(y.astype(np.int64))
    assert np.array_equal(counts.cpu().numpy(), want_counts[order])
    e_m = np.abs(means.cpu().numpy() - M.means_longdouble(xs, y)[order]) / M.mean_bound(want_counts[order], np.abs(xs).max())
    assert e_m.max() <= 1.0, e_m.max()
    want_s = _scatter_ref(n, d, k)
    e_s = float(np.abs(scatter.cpu().numpy() - want_s).max() / np.abs(want_s).max())
    print("world %d: merged scatter off by %.3g of max|S|" % (world, e_s))
    assert e_s <= SCATTER_TOL
    eng.fit_em_dev(means.data_ptr(), counts.data_ptr(), k, scatter.data_ptr(), d, iters)
    eng.synchronize()
    got = eng.get_model()
    one = MPlda(0)
    one.fit(xs, y, iters)
    ref = one.get_model()
    assert np.abs(got["psi"] - ref["psi"]).max() <= 1e-9 * ref["psi"].max()
    assert M.rel(got["transform"].T @ got["transform"], ref["transform"].T @ ref["transform"]) < 1e-9
    assert M.rel(got["mean"], ref["mean"]) < 1e-13
    orc, st = _fit_ref(n, d, k, iters)
    for m in (got, ref):
        T, psi = m["transform"], m["psi"]
        assert np.abs(psi - orc["psi"]).max() <= MODEL_TOL * orc["psi"].max()
        assert M.rel(T.T @ T, orc["transform"].T @ orc["transform"]) < MODEL_TOL
        assert M.rel(T.T @ np.diag(psi) @ T, orc["transform"].T @ np.diag(orc["psi"]) @ orc["transform"]) < MODEL_TOL
        assert np.abs(m["mean"] - (orc["mean"] + STATS_SHIFT)).max() <= M.model_mean_bound(st["counts"], np.abs(xs).max())
        assert np.abs(m["offset"] + T @ m["mean"]).max() <= 1e-12 * (np.abs(T) @ np.abs(m["mean"])).max()


# ----------------------------------------------------------------------------------------------------- (e) reproducibility, buffer reuse
@pytest.mark.parametrize("d", [33, 209, 210, 513])
def test_statistics_pass_on_offset_rows_is_bit_reproducible(d):
    from plda_amd import MPlda
    dd, n, k = next(s for s in M.STAT_SHAPES if s[0] == d)
    x, y = _data(n, d, k)
    a = _stats(MPlda(0), x + STATS_SHIFT, y, k)
    b = _stats(MPlda(0), x + STATS_SHIFT, y, k)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("d", [209, 210])
def test_statistics_pass_after_a_larger_one_on_the_same_handle(d):
    """D = 300, N = 900 first, then D = 209 / 210, N = 700 on the same handle: every scratch buffer of the pass (the centred rows
    among them) is larger than the second problem and full of the first one's values; the result is a fresh handle's, bit for bit."""
    from plda_amd import MPlda
    x1, y1 = _data(900, 300, 12)
    x2, y2 = _data(700, d, 9)
    eng = MPlda(0)
    first = _stats(eng, x1 + STATS_SHIFT, y1, 12)
    _check_stats(first, x1, y1, STATS_SHIFT, _scatter_ref(900, 300, 12), "before")
    again = _stats(eng, x2 + STATS_SHIFT, y2, 9)
    fresh = _stats(MPlda(0), x2 + STATS_SHIFT, y2, 9)
    for u, v in zip(again, fresh):
        assert np.array_equal(u, v)
    _check_stats(again, x2, y2, STATS_SHIFT, _scatter_ref(700, d, 9), "after", _PATH[d] != "gemm_f64_kernel")


# --------------------------------------------------------------------------------------------------------- (f) transform on offset rows
@pytest.mark.parametrize("d", [33, 209])
def test_transform_on_offset_rows(d):
    """A model whose mean carries the offset c (mean + c, the same T and psi; set_model derives offset = -T (mean + c)) transforms
    the rows x + c.  The kernel keeps Kaldi's  T x + offset,  two terms of size c that cancel, so it is held to the a-priori bound of
    that formula, fit_model.transform_bound (derived there: gamma_{D+1} (|T| |x| + |offset|) per component, carried through the
    length normalisation), against the same formula in extended precision on the arrays the library holds.
    tests/test_fit_model.py shows plain fp64 NumPy inside the same bound on the same inputs."""
    from plda_amd import MPlda
    x, n = M.transform_rows(d, 257, d)
    eng = MPlda(0)
    for c in M.SHIFTS:
        M.assert_exact_shift(x, c)
        mean, t, psi = M.transform_model(d + 1, d, c)
        eng.set_model(mean, t, psi)
        g = eng.get_model()
        assert np.array_equal(g["transform"], t) and np.array_equal(g["psi"], psi) and np.array_equal(g["mean"], mean)
        # the offset the library derived, inside the bound of its own dot product
        off_ref = -(t.astype(np.longdouble) @ mean.astype(np.longdouble))
        assert (np.abs(g["offset"] - off_ref) <= M.gamma(d) * (np.abs(t) @ np.abs(mean))).all()
        got = eng.transform_array(x + c, n)
        want, _, _ = M.transform_longdouble(t, g["offset"], psi, x + c, n)
        bound = M.transform_bound(t, g["offset"], psi, x + c, n)
        ratio = float((np.abs(got - want) / bound).max())
        print("D = %d shift %6d: transform error / bound = %.3g (bound %.3g of max|v|)" % (d, int(c), ratio, float(bound.max() / np.abs(want).max())))
        assert ratio <= 1.0, (c, ratio)
        one = eng.transform_array(x + c, 3)
        want1, _, _ = M.transform_longdouble(t, g["offset"], psi, x + c, np.full(len(x), 3))
        assert (np.abs(one - want1) <= M.transform_bound(t, g["offset"], psi, x + c, np.full(len(x), 3))).all()
