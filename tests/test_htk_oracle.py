"""CPU: the HTK oracle (oracle/htk_oracle_np.py) against the REFERENCE's own reader -- against the golden vectors
recorded from it (tests/golden/htk_cases.npz, and tests/golden/htk_live_cases.npz for the parametrised files below)
always, and live through oracle/_ref/libchtk_ref.so (the reference's chtk.cpp compiled where it lies) when the build
produced that library.  Bit-exact."""
import os

import numpy as np
import pytest

from oracle import htk_oracle_np as ho, ref_binding as rb

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "htk_cases.npz"))
CASES = sorted(k[:-5] for k in GOLD.files if k.endswith("_file"))
# the reference's header and frames for the files the two tests below write (tests/golden/make_htk_golden.py, live_cases)
LIVE = np.load(os.path.join(os.path.dirname(__file__), "golden", "htk_live_cases.npz"))


def _live_lib():
    """The reference's reader where the build compiled it (oracle/_ref is a build product, not every machine has one)."""
    return os.path.exists(rb.SO)


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_reference_golden(name):
    raw = GOLD[name + "_file"].tobytes()
    assert tuple(GOLD[name + "_header"]) == ho.load_header(raw)
    got = ho.htk_load(raw, int(GOLD[name + "_frm_ext"]))
    np.testing.assert_array_equal(got.ravel(), GOLD[name + "_out"])


@pytest.mark.parametrize("n,dim,f", [(0, 7, 2), (1, 1, 0), (3, 2, 5), (33, 24, 2), (120, 39, 0), (64, 64, 4)])
def test_oracle_matches_live_reference(tmp_path, n, dim, f):
    rng = np.random.default_rng(n * 131 + dim * 7 + f)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    p = str(tmp_path / "x.htk")
    ho.write_htk(p, x, sample_period=12345, parmkind=70)
    raw = open(p, "rb").read()
    key = "%d_%d_%d" % (n, dim, f)
    assert raw == LIVE[key + "_file"].tobytes()                  # the very file the reference read
    assert tuple(LIVE[key + "_header"]) == ho.load_header(raw)
    np.testing.assert_array_equal(ho.htk_load(raw, f).ravel(), LIVE[key + "_out"])
    if _live_lib():
        assert rb.header(p) == ho.load_header(raw)
        np.testing.assert_array_equal(ho.htk_load(raw, f).ravel(), rb.load(p, f))
    if f == 0:                                       # decode(encode(x)) == x, bit for bit
        np.testing.assert_array_equal(ho.htk_load(raw, 0).view(np.float32), x)


def test_negative_header_fields_follow_the_reference(tmp_path):
    raw = bytes([0xff, 0xff, 0xff, 0xfe, 0x80, 0, 0, 1, 0xff, 0xfc, 0x80, 0x01])
    assert raw == LIVE["negative_file"].tobytes()
    assert tuple(LIVE["negative_header"]) == ho.load_header(raw) == (-2, -(2 ** 31) + 1, -4, -32767)
    if _live_lib():
        p = str(tmp_path / "neg.htk")
        open(p, "wb").write(raw)
        assert rb.header(p) == ho.load_header(raw)


def test_bad_frame_size_is_rejected():
    with pytest.raises(ValueError):
        ho.htk_load(bytes([0, 0, 0, 1, 0, 0, 0, 1, 0, 6, 0, 9]) + b"\0" * 6, 0)
