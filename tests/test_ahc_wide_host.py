"""CPU: the Python side of the corpus-scale clustering (K28; plda_amd/diarize.py: ahc_wide, keep_clusters; MPlda.cluster_corpus,
MPlda.adapt_clustered) without a GPU: the argument checks, raised before any device work; the filter and renumber step against
its model (tests/ahc_wide_model.py); the constants and the methods of the three front ends."""
import ctypes as C
import inspect

import numpy as np
import pytest

import ahc_wide_model as W


class _NoDevice(object):
    """an engine whose every touch of the library fails the test: the checks must come first"""

    def __getattr__(self, name):
        raise AssertionError("device work before the argument check: %s" % name)


def _bare(cls):
    """an object of the class without a handle (no plda_create): any device call on it raises AttributeError"""
    return cls.__new__(cls)


def test_constants_and_signatures():
    from plda_amd import _native as N, diarize
    assert diarize.AHC_WIDE_MAX == 32768 and diarize.AHC_MAX == 4096
    i32, i64, f64, vp = C.c_int32, C.c_int64, C.c_double, C.c_void_p
    tail = [i32, f64, i32] + [vp] * 5
    assert N.SIGNATURES["plda_ahc_wide_plan"] == (C.c_int, [vp, i64, vp])
    for form in ("", "_dev"):
        assert N.SIGNATURES["plda_ahc_wide_matrix" + form] == (C.c_int, [vp, vp, i64, i64] + tail)
        assert N.SIGNATURES["plda_score_ahc_wide" + form] == (C.c_int, [vp, vp, i64] + tail)


def test_the_header_names_what_is_still_out_of_scope():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "plda_hip.h")) as f:
        text = f.read()
    assert "#define PLDA_AHC_WIDE_MAX 32768" in text and "corpus-scale clustering (K28" in text
    scope = text[text.index("OUT OF SCOPE, each on purpose: Kaldi's per-recording mean subtraction"):]
    scope = scope[:scope.index("---- */")]
    assert "several workgroups on one recording" not in scope
    assert "two-pass clustering" in scope and "PLDA_AHC_WIDE_MAX" in scope and "more than one GPU" in scope


def test_methods_exist_on_the_three_front_ends():
    from liblda.plda import PLDA
    from plda_amd import Cosine, MPlda
    for cls in (MPlda, PLDA, Cosine):
        for name in ("cluster_corpus", "adapt_clustered"):
            assert callable(getattr(cls, name)), (cls, name)
    assert Cosine.cluster_corpus is MPlda.cluster_corpus                  # inherited
    for cls in (MPlda, PLDA):
        assert list(inspect.signature(cls.cluster_corpus).parameters)[1:] == ["x", "threshold", "num_speakers", "return_merges"]
        sig = inspect.signature(cls.adapt_clustered)
        assert list(sig.parameters)[1:] == ["x", "threshold", "num_speakers", "alpha", "alpha_mean", "min_cluster_size", "iters"]
        assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [0.0, None, 0.5, None, 2, 10]
    with pytest.raises(ValueError, match="adapt_clustered needs a PLDA model"):
        _bare(Cosine).adapt_clustered(np.zeros((4, 2)))


def test_wide_args():
    from plda_amd import diarize
    assert diarize.wide_args(5, 0.0, None) == (1, 0.0, 1)
    assert diarize.wide_args(5, None, 3) == (0, 0.0, 3)
    assert diarize.wide_args(32768, -1.5, np.int64(2)) == (1, -1.5, 2)
    for n in (0, -1, 32769, True):
        with pytest.raises(ValueError, match="1 ... 32768"):
            diarize.wide_args(n, 0.0, None)
    with pytest.raises(ValueError, match="num_speakers"):
        diarize.wide_args(5, None, None)
    for ns in (0, -2, 1.5, [1, 2], True, np.asarray([1])):
        with pytest.raises(ValueError, match="num_speakers"):
            diarize.wide_args(5, 0.0, ns)
    for thr in (float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="threshold"):
            diarize.wide_args(5, thr, None)


def test_ahc_wide_checks_come_before_any_device_work():
    from plda_amd import diarize
    e = _NoDevice()
    for block in (np.zeros((3, 4), np.float32), np.zeros(9, np.float32), np.zeros((0, 0), np.float32), np.zeros((2, 2, 2), np.float32)):
        with pytest.raises(ValueError):
            diarize.ahc_wide(e, block)
    S = np.zeros((4, 4), np.float32)
    with pytest.raises(ValueError, match="num_speakers"):
        diarize.ahc_wide(e, S, threshold=None)
    with pytest.raises(ValueError, match="num_speakers"):
        diarize.ahc_wide(e, S, num_speakers=0)
    with pytest.raises(ValueError, match="NaN"):
        diarize.ahc_wide(e, S, threshold=float("nan"))
    with pytest.raises(ValueError):
        diarize.ahc_wide_vectors(e, np.zeros(8))
    with pytest.raises(ValueError, match="num_speakers"):
        diarize.ahc_wide_vectors(e, np.zeros((4, 2)), threshold=None)
    with pytest.raises(ValueError, match="1 ... 32768"):
        diarize.ahc_wide_vectors(e, np.zeros((0, 2)))


def test_cluster_corpus_and_adapt_clustered_checks_come_before_any_device_work():
    from plda_amd import MPlda
    m = _bare(MPlda)                                       # no handle: a device call would raise AttributeError
    x = np.zeros((6, 3))
    for bad in ([[0.0]], np.zeros(5), np.zeros((0, 3))):
        with pytest.raises(ValueError):
            m.cluster_corpus(bad)
    with pytest.raises(ValueError, match="num_speakers"):
        m.cluster_corpus(x, threshold=None)
    with pytest.raises(ValueError, match="num_speakers"):
        m.cluster_corpus(x, num_speakers=[2])
    with pytest.raises(ValueError, match="NaN"):
        m.cluster_corpus(x, threshold=float("nan"))
    for kw in (dict(min_cluster_size=0), dict(min_cluster_size=1.5), dict(iters=0), dict(alpha=1.5), dict(alpha=-0.1),
               dict(alpha_mean=2.0), dict(alpha="x"), dict(threshold=None), dict(num_speakers=0)):
        with pytest.raises(ValueError):
            m.adapt_clustered(x, **kw)


@pytest.mark.parametrize("seed", range(6))
def test_keep_clusters_equals_its_model(seed):
    from plda_amd import diarize
    rng = np.random.default_rng(seed)
    k = int(rng.integers(1, 40))
    labels = rng.integers(0, k, int(rng.integers(1, 400))).astype(np.int32)
    labels = np.searchsorted(np.unique(labels), labels).astype(np.int32)      # dense, as the clustering numbers them
    for m in (1, 2, 3, 7, 1000):
        rows, new, kept = diarize.keep_clusters(labels, m)
        wrows, wnew, wkept = W.keep_clusters(labels, m)
        assert rows.dtype == np.int64 and new.dtype == np.int64
        assert np.array_equal(rows, wrows) and np.array_equal(new, wnew) and kept == wkept
        if kept:
            assert sorted(set(new.tolist())) == list(range(kept)) and np.bincount(new).min() >= m
    assert diarize.keep_clusters(labels, 1)[0].tolist() == list(range(len(labels)))


def test_keep_clusters_edges():
    from plda_amd import diarize
    rows, new, kept = diarize.keep_clusters(np.asarray([2, 0, 2, 1, 2, 0], np.int32), 2)
    assert rows.tolist() == [0, 1, 2, 4, 5] and new.tolist() == [1, 0, 1, 1, 0] and kept == 2
    rows, new, kept = diarize.keep_clusters(np.zeros(0, np.int32), 2)
    assert rows.size == 0 and new.size == 0 and kept == 0
    for bad in (np.zeros((2, 2), np.int32), np.asarray([0.0, 1.0]), np.asarray([0, -1])):
        with pytest.raises(ValueError, match="labels"):
            diarize.keep_clusters(bad, 2)
    for m in (0, 1.5, True):
        with pytest.raises(ValueError, match="min_cluster_size"):
            diarize.keep_clusters(np.asarray([0, 1]), m)
