"""GPU: the HTK frame decoder (csrc/frontend.hip: htk_frames_kernel) through the device entry plda_htk_frames_dev at
every dispatch class -- word and 16-byte paths, the alignment fallbacks, every row-chunk size FR, the clamped context
at short files, chunk boundaries on and off file boundaries, and the 64-ary search of the frame offsets over the tables
of tests/frontend_model.py.  Every case is bit-exact against oracle.htk_oracle_np.htk_load per file.

File bodies are random 32-bit words (with signalling NaNs, -0 and subnormals planted in both byte orders), not floats:
every bit pattern must survive the copy.  The blob, both offset arrays and the output are guarded the way
tests/test_gpu_guard_bands.py guards its calls; the blob's neighbours hold the output's payload (or zero), and the
words between two files hold noise, so a read past a file's frames shows in the output."""
import struct

import numpy as np
import pytest

import frontend_model as fm
from test_gpu_guard_bands import GUARD_BYTES, PAYLOAD, _Output, _both, _dev, _input

pytestmark = pytest.mark.gpu

SPECIAL = np.array([0x7F800001, 0xFFA00000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7FC00000, 0x7F800000, 0xFFFFFFFF], np.uint32)
SPECIAL = np.concatenate([SPECIAL, SPECIAL.byteswap()])


@pytest.fixture(scope="module")
def eng():
    from plda_amd import MPlda
    return MPlda(0)


class _Batch:
    """Files of `counts` frames of W words; `pads[u]` words of noise in front of file u's data inside the blob."""

    def __init__(self, counts, w, seed=0, pads=None):
        rng = np.random.default_rng([seed, w])
        self.counts, self.w = [int(n) for n in counts], w
        pads = pads if pads is not None else [0] * len(self.counts)
        words, self.file_off, self.raw = [], [], []
        pos = 0
        for n, pad in zip(self.counts, pads):
            words.append(rng.integers(0, 2 ** 32, pad, dtype=np.uint32))
            pos += pad
            body = rng.integers(0, 2 ** 32, n * w, dtype=np.uint32)
            k = min(body.size, SPECIAL.size)
            body[:k] = SPECIAL[:k]
            self.file_off.append(pos)
            words.append(body)
            pos += body.size
            self.raw.append(struct.pack(">IIHH", n, 1, w * 4, 9) + body.astype("<u4").tobytes())
        self.words = np.concatenate(words + [rng.integers(0, 2 ** 32, 3, dtype=np.uint32)])
        self.frame_off = fm.offsets_of(self.counts)
        self.T = int(self.frame_off[-1])

    def expected(self, f):
        from oracle import htk_oracle_np as ho
        return np.concatenate([ho.htk_load(r, f) for r in self.raw])


def _blob(words, nan, shift_words=0):
    """The blob on the device, GUARD_BYTES of the payload (or zero) around it, `shift_words` past a 16-byte boundary."""
    import torch
    g = GUARD_BYTES // 4
    buf = torch.full((g + shift_words + words.size + g,), PAYLOAD if nan else 0, dtype=torch.int32, device=_dev())
    view = buf[g + shift_words:g + shift_words + words.size]
    view.copy_(torch.from_numpy(words.view(np.int32)).to(_dev()))
    assert view.data_ptr() % 16 == 4 * shift_words
    return buf, view


def _output(rows, cols, shift_words=0):
    """An _Output of float32 whose body starts `shift_words` past a 16-byte boundary."""
    import torch
    o = _Output(rows, cols, torch.float32)
    o.g += shift_words
    o.body = o.buf[o.g:o.g + rows * cols].view(rows, cols)
    assert o.ptr() % 16 == 4 * shift_words
    return o


def _decode(eng, b, f, out_shift=0, blob_shift=0):
    """Decode batch `b` with context f under NaN and zero neighbours and compare with the oracle, bit for bit."""
    def case(nan):
        import torch
        _, dblob = _blob(b.words, nan, blob_shift)
        _, dfile = _input(np.asarray(b.file_off, np.int64), nan)
        _, dframe = _input(b.frame_off, nan)
        out = _output(b.T, (2 * f + 1) * b.w, out_shift)
        torch.cuda.synchronize()
        eng._ck(eng._lib.plda_htk_frames_dev(eng._h, dblob.data_ptr(), dfile.data_ptr(), dframe.data_ptr(), len(b.counts), b.T,
                                             b.w * 4, f, out.ptr()))
        eng.synchronize()
        return dict(o=out.check("W=%d F=%d" % (b.w, f)).view(np.uint32))
    got = _both(case)["o"]
    want = b.expected(f)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, "W=%d F=%d: %d of %d frames differ, the first is frame %d" % (b.w, f, bad.size, b.T, bad[0])


MIXED = [5, 0, 1, 300, 2, 0, 0, 77, 1, 260, 33]


@pytest.mark.parametrize("w,f,counts", [(13, 0, MIXED), (13, 1, MIXED), (39, 2, MIXED), (1, 0, MIXED), (40, 0, MIXED), (8, 1, MIXED),
                                        (700, 6, [1, 3, 20]), (2048, 0, [1, 3, 20, 0, 6])])
def test_frame_sizes_and_row_chunks(eng, w, f, counts):
    """Word path (W % 4 != 0) at FR = 256, 210, 42 and the 256 cap; 16-byte path at FR = 204, 256, 1 (rows of 9100 words) and 4."""
    assert fm.chunk_frames(w, f) == {(13, 0): 256, (13, 1): 210, (39, 2): 42, (1, 0): 256, (40, 0): 204, (8, 1): 256,
                                     (700, 6): 1, (2048, 0): 4}[w, f]
    _decode(eng, _Batch(counts, w, seed=1), f)


@pytest.mark.parametrize("out_shift,blob_shift", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("f", [0, 2])
def test_pointers_only_four_byte_aligned(eng, f, out_shift, blob_shift):
    _decode(eng, _Batch(MIXED, 40, seed=2), f, out_shift, blob_shift)


@pytest.mark.parametrize("f", [0, 1])
def test_files_at_every_word_alignment_in_one_launch(eng, f):
    counts = [7, 30, 1, 0, 250, 12, 2, 90]
    want_mod = [0, 1, 2, 0, 3, 0, 2, 1]                  # file u's data starts at a word offset = want_mod[u] (mod 4)
    pads, pos = [], 0
    for n, m in zip(counts, want_mod):
        pad = (m - pos) % 4
        pads.append(pad)
        pos += pad + n * 40
    b = _Batch(counts, 40, seed=3, pads=pads)
    assert [o % 4 for o in b.file_off] == want_mod
    _decode(eng, b, f)


@pytest.mark.parametrize("w", [13, 40])
@pytest.mark.parametrize("f", [5, 0])
def test_context_clamped_at_short_files(eng, w, f):
    _decode(eng, _Batch([1, 2, 1, 1, 0, 2, 2, 1], w, seed=4), f)


@pytest.mark.parametrize("counts", [[204], [3 * 204 + 1], [204, 408, 204, 0, 204], [300, 312], [300, 313], [1] * 204 + [203, 1]])
def test_chunk_geometry(eng, counts):
    """W = 40, F = 0: chunks of FR = 204 frames.  A file of exactly FR frames, one of 3 FR + 1, file boundaries on
    multiples of FR, T = k FR and k FR + 1."""
    assert fm.chunk_frames(40, 0) == 204
    _decode(eng, _Batch(counts, 40, seed=5), 0)


@pytest.mark.parametrize("w,f", [(4, 0), (40, 1)])
@pytest.mark.parametrize("name", sorted(fm.search_tables()))
def test_search_of_the_frame_offsets(eng, name, w, f):
    """FR = 256 and 68: the chunk starts probe the 64-ary search at U = 1, 2, 64, 65, 66, 4097, across runs of 70 empty
    files first, in the middle and last, and over 5000 files of 0 and 1 frames in turn."""
    _decode(eng, _Batch(fm.search_tables()[name], w, seed=6), f)


def test_refusals_leave_the_handle_usable(eng):
    from plda_amd import _native as N
    b = _Batch([3, 0, 7], 8, seed=7)
    _, dblob = _blob(b.words, True)
    _, dfile = _input(np.asarray(b.file_off, np.int64), True)
    _, dframe = _input(b.frame_off, True)
    out = _output(b.T, 8)
    bp, fp, op, dp = dblob.data_ptr(), dfile.data_ptr(), dframe.data_ptr(), out.ptr()
    call = eng._lib.plda_htk_frames_dev
    bad = dict(samplesize6=(bp, fp, op, 3, b.T, 6, 0, dp), blob_plus_2=(bp + 2, fp, op, 3, b.T, 32, 0, dp),
               negative_context=(bp, fp, op, 3, b.T, 32, -1, dp), row_too_long=(bp, fp, op, 3, b.T, 4 << 18, 2, dp),
               no_blob=(None, fp, op, 3, b.T, 32, 0, dp), no_output=(bp, fp, op, 3, b.T, 32, 0, None))
    for what, args in bad.items():
        assert call(eng._h, *args) == N.PLDA_E_INVAL, what
        assert "htk_frames" in N.last_error(eng._h), what
    assert call(eng._h, bp, fp, op, 0, b.T, 32, 0, dp) == N.PLDA_OK               # U = 0
    assert call(eng._h, bp, fp, op, 3, 0, 32, 0, dp) == N.PLDA_OK                 # T = 0
    eng.synchronize()
    assert bool((out.words == PAYLOAD).all()), "a refused or empty call wrote to the output"
    _decode(eng, b, 1)                                                            # the handle still works
