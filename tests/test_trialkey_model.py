"""CPU: the trial key (include/plda_hip.h, "trial keys") without a GPU: plda_partition_plan against the NumPy statement
(tests/trialkey_model.py), its refusals, the new exports' signatures and the TrialKey rules."""
import ctypes as C

import numpy as np
import pytest

import trialkey_model as TM
from plda_amd import _native as N
from plda_amd import trialkey as TK

NEW_EXPORTS = ("plda_partition_plan", "plda_partition_matrix_dev", "plda_score_partition_dev", "plda_eer_lists_dev", "plda_det_lists_dev",
               "plda_min_dcf_lists_dev", "plda_calib_pass_lists_dev", "plda_calib_fit_lists_dev", "plda_rocch_lists_dev",
               "plda_fusion_pass_lists_dev", "plda_fusion_fit_lists_dev")


def _random_key(rng, m, nt, ce, ct, nb, p_none=0.3):
    table = rng.integers(0, nb, (ce, ct)).astype(np.int8)
    table[rng.random((ce, ct)) < p_none] = -1
    return rng.integers(0, ce, m).astype(np.uint8), rng.integers(0, ct, nt).astype(np.uint8), table


def _plan(ecode, tcode, table, nb, espk, tspk):
    key = TK.TrialKey.from_codes(ecode, tcode, table, list(range(nb)))
    return key.plan(espk, tspk)[0]


def _same(rec, model):
    count, offset, total = model
    assert np.array_equal(rec["count"], count) and np.array_equal(rec["offset"], offset) and np.array_equal(rec["total"], total)


def test_new_exports_and_signatures():
    lib = N.load()
    for name in NEW_EXPORTS:
        assert name in N.SIGNATURES and hasattr(lib, name), name
    for dev in NEW_EXPORTS[3:]:
        # a device-list form takes its host-list sibling's arguments
        assert N.SIGNATURES[dev] == N.SIGNATURES[dev[:-4]], dev
    assert N.SIGNATURES["plda_score_partition_dev"][1][:11] == N.SIGNATURES["plda_score_eer_dev"][1][:11]
    assert lib.plda_abi_version() == 2
    assert (TK.MAX_CODES, TK.MAX_BUCKETS, TK.STRIP) == (128, 8, 256)


@pytest.mark.parametrize("seed", range(6))
def test_plan_equals_the_model_on_random_keys(seed):
    rng = np.random.default_rng(seed)
    m, nt = int(rng.integers(1, 90)), int(rng.integers(1, 700))
    ce, ct, nb = int(rng.integers(1, 9)), int(rng.integers(1, 9)), int(rng.integers(1, 9))
    ecode, tcode, table = _random_key(rng, m, nt, ce, ct, nb)
    # duplicate speakers on both sides, speakers of one side only
    espk = rng.integers(0, 12, m).astype(np.int64) * 7 - 20
    tspk = rng.integers(6, 20, nt).astype(np.int64) * 7 - 20
    _same(_plan(ecode, tcode, table, nb, espk, tspk), TM.plan(ecode, tcode, table, nb, espk, tspk))


def test_plan_edges():
    rng = np.random.default_rng(7)
    m, nt = 40, 300
    espk, tspk = rng.integers(0, 9, m).astype(np.int64), rng.integers(0, 9, nt).astype(np.int64)
    # every pair masked
    ecode, tcode, table = _random_key(rng, m, nt, 3, 4, 2)
    table[:] = -1
    rec = _plan(ecode, tcode, table, 2, espk, tspk)
    assert not rec["count"].any() and not rec["total"].any() and not rec["offset"].any()
    # an empty bucket in the middle, a bucket with no target (its codes' speakers never meet), 128 codes per side
    ecode, tcode = (np.arange(m) % 128).astype(np.uint8), (np.arange(nt) % 128).astype(np.uint8)
    table = np.full((128, 128), -1, np.int8)
    table[:64, :64], table[64:, 64:] = 0, 2
    rec = _plan(ecode, tcode, table, 4, espk, tspk)
    _same(rec, TM.plan(ecode, tcode, table, 4, espk, tspk))
    assert rec["count"][1].sum() == 0 and rec["count"][3].sum() == 0 and rec["count"][0].sum() > 0
    no_tar = _plan(ecode, tcode, table, 4, espk, tspk + 100)
    assert no_tar["total"][1] == 0 and no_tar["total"][0] == rec["total"].sum()
    # extreme ids
    big = np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0, -1], np.int64)
    e, t = big[rng.integers(0, 4, m)], big[rng.integers(0, 4, nt)]
    _same(_plan(ecode, tcode, table, 4, e, t), TM.plan(ecode, tcode, table, 4, e, t))


def _raw_plan(espk, tspk, ecode, tcode, table, ce, ct, nb, rec=True):
    out = np.full(1, -7, TK.RECORD_DTYPE)
    key = TK._Key(ecode.ctypes.data if ecode is not None else None, tcode.ctypes.data if tcode is not None else None,
                  table.ctypes.data if table is not None else None, ce, ct, nb, 0)
    rc = N.load().plda_partition_plan(C.c_void_p(espk.ctypes.data), espk.shape[0], C.c_void_p(tspk.ctypes.data), tspk.shape[0],
                                      C.cast(C.byref(key), C.c_void_p), C.c_void_p(out.ctypes.data) if rec else None)
    return rc, out, N.last_error(None)


def test_plan_refusals_write_nothing():
    espk, tspk = np.arange(5, dtype=np.int64), np.arange(9, dtype=np.int64)
    ecode, tcode = np.zeros(5, np.uint8), np.zeros(9, np.uint8)
    ok = np.zeros((2, 2), np.int8)
    rc, out, _ = _raw_plan(espk, tspk, ecode, tcode, ok, 2, 2, 1)
    assert rc == N.PLDA_OK and out[0]["total"][0] + out[0]["total"][1] == 45
    untouched = np.full(1, -7, TK.RECORD_DTYPE)
    bad_e, bad_t = ecode.copy(), tcode.copy()
    bad_e[3], bad_t[8] = 2, 200
    cases = [
        (dict(ecode=bad_e), "enrol_code[3]"), (dict(tcode=bad_t), "test_code[8]"),
        (dict(table=np.array([[0, 1], [0, 0]], np.int8)), "table entry (0, 1)"), (dict(table=np.array([[0, -2], [0, 0]], np.int8)), "table entry"),
        (dict(ce=0), "codes"), (dict(ce=129), "codes"), (dict(ct=129), "codes"), (dict(nb=0), "buckets"), (dict(nb=9), "buckets"),
        (dict(table=None), "NULL"), (dict(ecode=None), "NULL"), (dict(rec=False), "bad argument"),
    ]
    for change, text in cases:
        args = dict(espk=espk, tspk=tspk, ecode=ecode, tcode=tcode, table=ok, ce=2, ct=2, nb=1)
        args.update(change)
        rc, out, msg = _raw_plan(**args)
        assert rc == N.PLDA_E_INVAL and text in msg, (change, msg)
        assert out.tobytes() == untouched.tobytes(), change
    rc, out, msg = _raw_plan(espk[:0], tspk, ecode[:0], tcode, ok, 2, 2, 1)
    assert rc == N.PLDA_E_INVAL and out.tobytes() == untouched.tobytes()


def test_trialkey_rules():
    eg, tg = np.array(["f", "m", "m", "f", "x"]), np.array(["m", "f", "f", "m", "m", "y"])
    same = TK.TrialKey(eg, tg, "same")
    assert same.bucket_names == ["f", "m"] and same.n_buckets == 2 and same.shape == (5, 6)
    mask = same.mask()
    for i, e in enumerate(eg):
        for j, t in enumerate(tg):
            assert mask[i, j] == (same.bucket_names.index(e) if e == t else -1)
    every = TK.TrialKey(eg, tg, "all")
    assert every.bucket_names == ["all"] and (every.mask() == 0).all() and every.mask().shape == (5, 6)
    assert (TK.TrialKey(3, 4, "all").mask() == 0).all()
    rule = {("f", "m"): "cross", ("m", "f"): "cross", ("f", "f"): "ff", ("zz", "m"): "never"}
    mapped = TK.TrialKey(eg, tg, rule)
    assert mapped.bucket_names == ["cross", "ff", "never"]
    mm = mapped.mask()
    for i, e in enumerate(eg):
        for j, t in enumerate(tg):
            want = rule.get((e, t))
            assert mm[i, j] == (mapped.bucket_names.index(want) if want is not None else -1)
    with pytest.raises(ValueError):
        TK.TrialKey(eg, tg, "other")
    with pytest.raises(ValueError, match="buckets"):
        TK.TrialKey(np.arange(9), np.arange(9), "same")
    with pytest.raises(ValueError, match="labels"):
        TK.TrialKey(np.arange(129), np.arange(3), {})
    # the library agrees with the key's own mask
    espk, tspk = np.array([1, 2, 3, 1, 2], np.int64), np.array([2, 1, 9, 1, 2, 3], np.int64)
    rec = mapped.plan(espk, tspk)[0]
    _same(rec, TM.plan(mapped.enrol_code, mapped.test_code, mapped.table, mapped.n_buckets, espk, tspk))
    with pytest.raises(ValueError):
        mapped.plan(espk[:4], tspk)


def test_trialkey_product():
    rng = np.random.default_rng(3)
    m, nt = 17, 23
    eg, tg = rng.integers(0, 2, m), rng.integers(0, 2, nt)
    el, tl = rng.integers(0, 3, m), rng.integers(0, 3, nt)
    k1, k2 = TK.TrialKey(eg, tg, "same"), TK.TrialKey(el, tl, "same")
    kp = TK.TrialKey.product(k1, k2)
    assert kp.n_buckets == 6 and kp.bucket_names == [(a, b) for a in (0, 1) for b in (0, 1, 2)]
    m1, m2, mp = k1.mask().astype(int), k2.mask().astype(int), kp.mask().astype(int)
    assert np.array_equal(mp, np.where((m1 >= 0) & (m2 >= 0), m1 * 3 + m2, -1))
    assert kp.enrol_code.dtype == np.uint8 and kp.table.dtype == np.int8
    with pytest.raises(ValueError, match="buckets"):
        TK.TrialKey.product(kp, k1)
    wide = TK.TrialKey(np.arange(m) % 12, np.arange(nt) % 12, {(0, 0): "a"})
    with pytest.raises(ValueError, match="codes"):
        TK.TrialKey.product(wide, wide)
    with pytest.raises(ValueError, match="different"):
        TK.TrialKey.product(k1, TK.TrialKey(eg[:5], tg, "same"))
