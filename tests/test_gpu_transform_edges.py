"""GPU: K4, the batched Plda::TransformIvector (csrc/transform.hip), at its edges -- against the np.longdouble model of the
DEFINITION t = T (x - mean) and its derived forward bound (tests/transform_model.py; tests/test_transform_model.py shows on the
host that the rule is sound and rejects planted faults).  THE RULE, for every case: each element within B (no factor), the
normaliser residual rho within (Dout + 24) u, all copies of a pool entry inside one launch bit-identical, and no row excluded.

Rows come from a pool of 61 distinct (row, n) entries spread over the launch by a seeded index; the longdouble reference is
computed for the pool alone.  Which block shapes a row count reaches is read from plda_transform_plan and ASSERTED: per
dimension class and count form the main shape and every tail shape run, by name.

With TRANSFORM_PARITY_JSON set the per-case figures -- deviation / B, rho in units of u, the device's deviation over a NumPy
fp64 evaluation's -- are written there (profiles/transform_parity.json is such a file).  Worst figures on an MI355X (256 CUs),
over its 48 cases: deviation 0.149 B (Din = Dout = 3, per-row counts), residual 7.1 u (the same case; the bound there is 27 u),
1.87 times NumPy's deviation (512 x 512, |mean| = 1e6 spreads).  B / |out| on offset data, median: 6.1e-10 (Dout = 208) and
2.3e-9 (512) at |mean| = 1e3 spreads, 6.1e-7 and 2.3e-6 at 1e6.  No bound was broken.

Nothing here provokes a fault: every bad value (a NaN, an Inf, a zero row, a count <= 0) sits in a buffer the test owns, and the
guard bands around the outputs are the test's own memory."""
import json
import os

import numpy as np
import pytest

import transform_model as M

pytestmark = pytest.mark.gpu

E_INVAL = -1
CLASS_EDGES = [(130, 128), (211, 208), (257, 256), (389, 384), (512, 512)]       # the upper edge of every class, ragged Din
COUNTS = (1, 2, 3, 5, 8, 100)
_PARITY = {}


def _dev():
    import torch
    return torch.device("cuda", 0)


def _engine(monkeypatch, variant="0"):
    from plda_amd import MPlda
    monkeypatch.setenv("PLDA_TRANSFORM_VARIANT", variant)
    return MPlda(0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _run(eng, dx, n, dout):
    """transform_rows_dev on the device rows dx with counts n (an int: uniform; a device int32 tensor: per row) -> host array"""
    import torch
    r, din = dx.shape
    out = torch.empty((r, dout), dtype=torch.float64, device=_dev())
    torch.cuda.synchronize()
    if isinstance(n, (int, np.integer)):
        eng.transform_rows_dev(dx.data_ptr(), r, din, None, int(n), out.data_ptr())
    else:
        eng.transform_rows_dev(dx.data_ptr(), r, din, n.data_ptr(), 0, out.data_ptr())
    eng.synchronize()
    return out.cpu().numpy()


def _record(name, fig):
    _PARITY[name] = fig
    worst = {k: max(v[k] for v in _PARITY.values() if k in v) for k in ("dev", "rho", "dev_over_numpy")}
    path = os.environ.get("TRANSFORM_PARITY_JSON")
    if path:
        with open(path, "w") as f:
            json.dump({"cases": _PARITY, "worst": worst}, f, indent=1, sort_keys=True)


class _Pool(object):
    """A model, its pool of 61 (row, n) entries and the pool's longdouble reference, for one count form."""

    def __init__(self, model, x, n, form, uniform=3):
        self.model, self.x, self.n, self.form, self.uniform = model, x, n, form, uniform
        self.dout, self.din = model[1].shape
        self.refer()

    def refer(self):
        """the longdouble reference of the pool as it stands, and a NumPy fp64 evaluation's deviation from it"""
        mean, T, psi = self.model
        self.counts = self.n if self.form == "perrow" else self.uniform
        self.ref = M.model(T, mean, psi, self.x, self.counts)
        M.assert_well_posed(self.ref, "pool %dx%d" % (self.din, self.dout))          # no row is excluded: before the device runs
        self.numpy_dev = float(np.max(M.deviation(M.offset_form(T, mean, psi, self.x, self.counts), self.ref)))
        self.dx, self.dn = _t(self.x), _t(self.n)

    def run(self, eng, r, what, seed=0):
        """r rows spread from the pool through the device; copies bit-identical per launch; the rule on one copy per launch and
        entry -> (figures, plan)"""
        import torch
        plan = eng.transform_plan(r)
        idx = M.spread_index(np.random.default_rng([self.din, self.dout, r, seed]), r)
        didx = _t(idx)
        dx = self.dx[didx]
        dn = self.dn[didx] if self.form == "perrow" else int(self.counts)
        torch.cuda.synchronize()
        got = _run(eng, dx, dn, self.dout)
        rows, entries = M.assert_copies_identical(got, idx, plan, what)
        cnt = self.n[entries] if self.form == "perrow" else self.counts
        fig = M.assert_rule(got[rows], self.ref, self.model[2], cnt, what, rows=entries)
        fig["dev_over_numpy"] = fig["dev"] / self.numpy_dev
        return fig, plan


def _pool(din, dout, form, seed, mean_size=1.0, counts=COUNTS, uniform=3):
    """a drawn model and pool"""
    rng = np.random.default_rng([din, dout, seed])
    model = M.make_model(rng, din, dout, mean_size)
    x, n = M.pool_rows(rng, din, model[0], counts)
    return _Pool(model, x, n, form, uniform)


def _ladder(eng, pool, rs, name):
    eng.set_model(*pool.model)
    shapes, worst = set(), {}
    for r in rs:
        fig, plan = pool.run(eng, r, "%s R = %d" % (name, r))
        assert plan["main_rows"] + plan["tail_rows"] == r
        shapes |= M.shapes_of(plan)
        worst = {k: max(fig[k], worst.get(k, 0.0)) for k in fig}
    print("%s: deviation %.3g B, residual %.2f u, %.2f of NumPy's deviation; shapes %s" % (name, worst["dev"], worst["rho"], worst["dev_over_numpy"], sorted(shapes)))
    _record(name, worst)
    return shapes


# ------------------------------------------------------------------------------------------- every instantiation, by name
@pytest.mark.parametrize("form", ["uniform", "perrow"])
@pytest.mark.parametrize("din,dout", CLASS_EDGES)
def test_every_block_shape_of_every_class(monkeypatch, din, dout, form):
    """The upper edge of every dimension class with a ragged Din, both count forms; the row counts come from the plan (G compute
    units, ROWS0 rows in a main block) and reach the main shape, every tail shape of the class and the main shape as a tail --
    asserted on the plans, so a device with another CU count cannot quietly run fewer shapes."""
    eng = _engine(monkeypatch)
    pool = _pool(din, dout, form, seed=1)
    eng.set_model(*pool.model)
    p1 = eng.transform_plan(1)
    g, rows0 = p1["cus"], p1["main_block"]
    assert p1["arm"] == "fused" and p1["cls"] == CLASS_EDGES.index((din, dout)) and rows0 == (128 if dout <= 256 else 64)
    rs = [1, 15, 16, 17, 16 * g, 16 * g + 1, 32 * g + 1, 64 * g + 1, rows0 * g, rows0 * g + 1, rows0 * g + 16 * g + 1]
    shapes = _ladder(eng, pool, rs, "edge %dx%d %s" % (din, dout, form))
    tails = (16, 32, 64, 128) if rows0 == 128 else (16, 32, 64)              # (the last: the main shape used as a tail)
    assert shapes == {("main", rows0)} | {("tail", b) for b in tails}, shapes
    # exactly one round and no tail; one row more: a tail of one 16-row block
    assert eng.transform_plan(rows0 * g)["tail_rows"] == 0 and eng.transform_plan(rows0 * g + 1)["tail_rows"] == 1


@pytest.mark.parametrize("form", ["uniform", "perrow"])
@pytest.mark.parametrize("dout", [129, 209, 257, 385])
def test_lower_class_edges(monkeypatch, dout, form):
    """one column past a class edge: the next class with its last column tiles almost empty"""
    eng = _engine(monkeypatch)
    pool = _pool(dout + 3, dout, form, seed=2)
    eng.set_model(*pool.model)
    p1 = eng.transform_plan(1)
    assert p1["cls"] == [129, 209, 257, 385].index(dout) + 1
    _ladder(eng, pool, [1, 17, 16 * p1["cus"] + 1], "lower edge %dx%d %s" % (dout + 3, dout, form))


@pytest.mark.parametrize("form", ["uniform", "perrow"])
@pytest.mark.parametrize("d", [1, 3, 4, 13, 16, 17])
def test_small_depths(monkeypatch, d, form):
    """contractions of less than one k-step, one k-step, one stage and one stage plus one"""
    eng = _engine(monkeypatch)
    _ladder(eng, _pool(d, d, form, seed=3), [17], "depth %d %s" % (d, form))


@pytest.mark.parametrize("form", ["uniform", "perrow"])
@pytest.mark.parametrize("din,dout,variant", [(520, 520, "0"), (513, 513, "0"), (211, 208, "1")])
def test_pair_arm(monkeypatch, din, dout, variant, form):
    """the GEMM + length-norm pair: Dout > 512, and forced at a dimension the one-pass kernel takes"""
    eng = _engine(monkeypatch, variant)
    pool = _pool(din, dout, form, seed=4)
    eng.set_model(*pool.model)
    assert eng.transform_plan(257) == {"arm": "pair", "cls": -1, "main_rows": 257, "main_block": 4, "tail_rows": 0, "tail_block": 0,
                                       "cus": eng.transform_plan(1)["cus"]}
    _ladder(eng, pool, [1, 63, 64, 257], "pair %dx%d %s" % (din, dout, form))


def test_plan_arguments(monkeypatch):
    from plda_amd import MPlda
    from plda_amd._native import PldaError
    eng = MPlda(0)
    with pytest.raises(PldaError):
        eng.transform_plan(1)                                   # no model
    eng.set_model(*M.make_model(np.random.default_rng(0), 20, 20))
    with pytest.raises(PldaError, match="R = -1"):
        eng.transform_plan(-1)
    p0 = eng.transform_plan(0)
    assert (p0["main_rows"], p0["tail_rows"], p0["tail_block"]) == (0, 0, 0)
    out = (np.zeros(8, np.int64))
    assert eng._lib.plda_transform_plan(eng._h, 5, None) == E_INVAL
    assert eng._lib.plda_transform_plan(eng._h, 5, out.ctypes.data) == 0 and out[4] == 5 and out[5] == 16 and out[7] == 0


def _cus(eng, pool):
    eng.set_model(*pool.model)
    return eng.transform_plan(1)["cus"]


# ------------------------------------------------------------------------------------------- value edges
VALUE_SHAPES = [(211, 208, "0"), (512, 512, "0"), (211, 208, "1"), (512, 512, "1")]     # Dout = 208 and 512, both arms


def _value_rows(eng, arm):
    """row counts that reach every block shape of the class (the pair arm has one shape: a short ladder)"""
    p1 = eng.transform_plan(1)
    g, rows0 = p1["cus"], p1["main_block"]
    return [1, 63, 257] if arm == "1" else [17, 16 * g + 1, 32 * g + 1, 64 * g + 1, rows0 * g + 1]


@pytest.mark.parametrize("mean_size", [1e3, 1e6])
@pytest.mark.parametrize("din,dout,variant", VALUE_SHAPES)
def test_offset_data(monkeypatch, din, dout, variant, mean_size):
    """|mean| = 1e3 and 1e6 times the spread of the rows: within B, which grows with |mean| -- B / |out| is recorded, it is the
    sentence about an offset mean in include/plda_hip.h."""
    eng = _engine(monkeypatch, variant)
    pool = _pool(din, dout, "perrow", seed=5, mean_size=mean_size)
    name = "offset %g %dx%d arm %s" % (mean_size, din, dout, variant)
    _ladder(eng, pool, [17, 16 * _cus(eng, pool) + 1], name)
    rel = pool.ref["B"] / np.abs(pool.ref["out"])
    _PARITY[name]["B_over_out_median"] = float(np.median(rel))
    _record(name, _PARITY[name])
    print("%s: B / |out| median %.3g" % (name, float(np.median(rel))))


@pytest.mark.parametrize("din,dout,variant", VALUE_SHAPES)
def test_row_scales(monkeypatch, din, dout, variant):
    """rows scaled by 1e-100 and 1e+100 beside ordinary ones (mean = 0, so the scale reaches t): the norm is per row and the
    sum of squares stays inside the fp64 range -- within B like any other row"""
    eng = _engine(monkeypatch, variant)
    pool = _pool(din, dout, "perrow", seed=6, mean_size=0.0)
    pool.x[1::3] *= 1e-100
    pool.x[2::3] *= 1e100
    pool.refer()
    _ladder(eng, pool, [17, 16 * _cus(eng, pool) + 1], "scales %dx%d arm %s" % (din, dout, variant))


def _special_positions(plan):
    r = plan["main_rows"] + plan["tail_rows"]
    pos = {0, 15, 16, r - 1}                       # r - 1: the row the loads of the rows past R are clamped to
    if plan["main_rows"]:
        pos |= {plan["main_rows"] - 1}
    if plan["main_rows"] and plan["tail_rows"]:
        pos |= {plan["main_rows"]}
    return sorted(p for p in pos if 0 <= p < r)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("kind", ["zero", "nan", "inf"])
@pytest.mark.parametrize("din,dout,variant", VALUE_SHAPES)
def test_rows_without_a_direction(monkeypatch, din, dout, variant, kind):
    """A zero row under mean = 0 (t = 0 exactly), and one NaN or one Inf element: in rows 0, 15, 16, the last row of the main
    launch, the first of the tail and row R - 1, under every block shape.  Those rows come back all NaN, every other row is
    bit-identical to the clean run."""
    import torch
    eng = _engine(monkeypatch, variant)
    pool = _pool(din, dout, "perrow", seed=7, mean_size=0.0)
    eng.set_model(*pool.model)
    for r in _value_rows(eng, variant):
        plan = eng.transform_plan(r)
        idx = _t(M.spread_index(np.random.default_rng(r), r))
        dx, dn = pool.dx[idx].clone(), pool.dn[idx]
        clean = _run(eng, dx, dn, dout)
        assert np.isfinite(clean).all()
        pos = _special_positions(plan)
        for k, p in enumerate(pos):
            if kind == "zero":
                dx[p] = 0.0
            else:
                dx[p, (37 * k + din - 1) % din] = float("nan") if kind == "nan" else float("inf") * (-1) ** k
        torch.cuda.synchronize()
        got = _run(eng, dx, dn, dout)
        keep = np.ones(r, bool)
        keep[pos] = False
        assert np.isnan(got[~keep]).all(), "%s rows, R = %d: %d elements are not NaN" % (kind, r, int((~np.isnan(got[~keep])).sum()))
        assert _same_bits(got[keep], clean[keep]), "%s rows, R = %d: a neighbour changed" % (kind, r)


@pytest.mark.parametrize("din,dout,variant", VALUE_SHAPES)
def test_a_row_equal_to_the_mean_leaves_its_neighbours_alone(monkeypatch, din, dout, variant):
    """x = mean != 0 has no meaningful direction (t is rounding residue): only the neighbours are asserted"""
    eng = _engine(monkeypatch, variant)
    pool = _pool(din, dout, "perrow", seed=8)
    eng.set_model(*pool.model)
    dmean = _t(pool.model[0])
    for r in _value_rows(eng, variant)[:2]:
        idx = _t(M.spread_index(np.random.default_rng(r), r))
        dx, dn = pool.dx[idx].clone(), pool.dn[idx]
        clean = _run(eng, dx, dn, dout)
        pos = _special_positions(eng.transform_plan(r))
        dx[pos] = dmean
        got = _run(eng, dx, dn, dout)
        keep = np.ones(r, bool)
        keep[pos] = False
        assert _same_bits(got[keep], clean[keep])


@pytest.mark.parametrize("c", [1, 2, 4095, 4096, 5000, 2 ** 31 - 1])
@pytest.mark.parametrize("din,dout,variant", VALUE_SHAPES)
def test_extreme_counts_and_the_two_count_forms_agree(monkeypatch, din, dout, variant, c):
    """a per-row array holding one value c gives the uniform count c's bits: the code forms the same weights and sums them in the
    same order; both within B of the model"""
    import torch
    eng = _engine(monkeypatch, variant)
    pool = _pool(din, dout, "uniform", seed=9, uniform=c)
    eng.set_model(*pool.model)
    p1 = eng.transform_plan(1)
    rs = [1, 63, 257] if variant == "1" else [17, 16 * p1["cus"] + 1, p1["main_block"] * p1["cus"] + 1]
    for r in rs:
        idx = M.spread_index(np.random.default_rng(r), r)
        dx = pool.dx[_t(idx)]
        dn = torch.full((r,), c, dtype=torch.int32, device=_dev())
        uni, per = _run(eng, dx, c, dout), _run(eng, dx, dn, dout)
        assert _same_bits(uni, per), "count %d, R = %d: the two count forms differ in bits" % (c, r)
        rows, entries = M.assert_copies_identical(uni, idx, eng.transform_plan(r))
        M.assert_rule(uni[rows], pool.ref, pool.model[2], c, "count %d R = %d" % (c, r), rows=entries)


# ------------------------------------------------------------------------------------------- counts <= 0
@pytest.mark.parametrize("din,dout,variant", VALUE_SHAPES)
def test_counts_not_above_zero_on_the_device_form(monkeypatch, din, dout, variant):
    """transform_rows_dev: a row whose count is 0 or -1 (or INT32_MIN) comes back all NaN, its neighbours are bit-identical to the
    clean run; inputs and outputs sit between guard bands (tests/test_gpu_guard_bands.py), NaN and zero neighbours alike"""
    import torch
    from test_gpu_guard_bands import _Output, _both, _input
    eng = _engine(monkeypatch, variant)
    pool = _pool(din, dout, "perrow", seed=10)
    eng.set_model(*pool.model)
    for r in _value_rows(eng, variant)[:3]:
        idx = M.spread_index(np.random.default_rng(r), r)
        x, n = pool.x[idx], pool.n[idx].copy()
        pos = _special_positions(eng.transform_plan(r))
        bad = n.copy()
        bad[pos] = np.array([0, -1, -2 ** 31, 0, -1, 0, -1])[:len(pos)]

        def case(nan):
            _, dx = _input(x, nan)
            _, dn = _input(n, nan)
            _, db = _input(bad, nan)
            o1, o2 = _Output(r, dout, torch.float64), _Output(r, dout, torch.float64)
            torch.cuda.synchronize()
            eng.transform_rows_dev(dx.data_ptr(), r, din, dn.data_ptr(), 0, o1.ptr())
            eng.transform_rows_dev(dx.data_ptr(), r, din, db.data_ptr(), 0, o2.ptr())
            eng.synchronize()
            return dict(clean=o1.check("clean"), bad=o2.check("counts <= 0"))

        a = _both(case)
        keep = np.ones(r, bool)
        keep[pos] = False
        assert np.isfinite(a["clean"]).all() and np.isnan(a["bad"][~keep]).all()
        assert _same_bits(a["bad"][keep], a["clean"][keep])


def test_counts_not_above_zero_on_the_host_form(monkeypatch):
    """plda_transform_rows counts them on the host: PLDA_E_INVAL with the count in plda_last_error, nothing written, the handle
    keeps working; transform_array raises ValueError; a uniform count <= 0 is PLDA_E_INVAL in both forms"""
    import torch
    from plda_amd._native import PldaError, last_error
    eng = _engine(monkeypatch)
    pool = _pool(33, 17, "perrow", seed=11)
    eng.set_model(*pool.model)
    x = np.ascontiguousarray(pool.x)
    n = pool.n.copy()
    want = eng.transform_array(x, n)
    bad = n.copy()
    bad[[3, 7, 60]] = [0, -1, -5]
    out = np.full((M.POOL, 17), 7.25)
    rc = eng._lib.plda_transform_rows(eng._h, x.ctypes.data, M.POOL, 33, bad.ctypes.data, 0, out.ctypes.data)
    assert rc == E_INVAL and "3 of 61 rows" in last_error(eng._h) and "row 3" in last_error(eng._h), last_error(eng._h)
    assert (out == 7.25).all()                                            # nothing is written
    with pytest.raises(ValueError, match="3 of 61"):
        eng.transform_array(x, bad)
    for nu in (0, -1):
        assert eng._lib.plda_transform_rows(eng._h, x.ctypes.data, M.POOL, 33, None, nu, out.ctypes.data) == E_INVAL
        dx = _t(x)
        dout = torch.full((M.POOL, 17), 7.25, dtype=torch.float64, device=_dev())
        with pytest.raises(PldaError):
            eng.transform_rows_dev(dx.data_ptr(), M.POOL, 33, None, nu, dout.data_ptr())
        eng.synchronize()
        assert bool((dout == 7.25).all()) and (out == 7.25).all()
    assert _same_bits(eng.transform_array(x, n), want)                    # the handle keeps working


# ------------------------------------------------------------------------------------------- transform_groups
def _groups_reference(model, x, labels):
    """per group (ascending label): the count, the longdouble mean, and the bound of the device's fp64 mean -- a sum of count
    terms in any order carries at most (count - 1) u sum |x_i|, the division u |mean|: together at most u sum_i |x_ik|"""
    keys = np.unique(labels)
    xl = x.astype(M.LD)
    means = np.stack([xl[labels == k].mean(0) for k in keys])
    dx = np.stack([M.U * np.abs(xl[labels == k]).sum(0) for k in keys])
    counts = np.array([(labels == k).sum() for k in keys], np.int64)
    mean, T, psi = model
    return keys, counts, M.model(T, mean, psi, means, counts, dx=dx)


@pytest.mark.parametrize("identity", [False, True])
@pytest.mark.parametrize("shape", ["one group", "every row its own", "N = 1", "mixed"])
def test_transform_groups(monkeypatch, shape, identity):
    """plda_transform_groups at its group shapes, with the label values 0 and 2^64 - 1: ascending order, the counts, and the vectors
    under the rule with the group's count.  The group means are not an output; they are judged through the vectors, whose bound
    takes the mean's own rounding as an input error -- sharply so with T = I, mean = 0 (`identity`), where the vector IS the
    normalised group mean."""
    eng = _engine(monkeypatch)
    din = 72
    rng = np.random.default_rng([len(shape), identity])
    model = M.make_model(rng, din, din)
    if identity:
        model = (np.zeros(din), np.eye(din), model[2])
    eng.set_model(*model)
    big = np.uint64(2 ** 64 - 1)
    if shape == "one group":
        x, labels = 1.0 + rng.standard_normal((700, din)), np.full(700, big, np.uint64)
    elif shape == "every row its own":
        x = rng.standard_normal((300, din))
        labels = rng.permutation(300).astype(np.uint64) * np.uint64(7919)
        labels[labels == labels.max()] = big                              # (0 is among them: the permutation holds it)
    elif shape == "N = 1":
        x, labels = rng.standard_normal((1, din)), np.zeros(1, np.uint64)
    else:
        x = 0.5 + rng.standard_normal((900, din))
        labels = rng.integers(0, 40, 900).astype(np.uint64) * np.uint64(2 ** 58 + 13)
        labels[labels == labels.max()] = big
    keys, counts, ref = _groups_reference(model, x, labels)
    M.assert_well_posed(ref, shape)
    got = eng.transform(x, labels)
    assert list(got.keys()) == [int(k) for k in keys]                     # ascending, 0 first and 2^64 - 1 last where present
    assert (0 in got) == (shape != "one group") and (int(big) in got) == (shape != "N = 1")
    assert [got[int(k)][0] for k in keys] == counts.tolist()
    vecs = np.stack([got[int(k)][1] for k in keys])
    fig = M.assert_rule(vecs, ref, model[2], counts, shape)
    print("groups %s%s: deviation %.3g B, residual %.2f u" % (shape, ", T = I" if identity else "", fig["dev"], fig["rho"]))
