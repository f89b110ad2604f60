"""tests/transform_model.py -- a np.longdouble model of K4, the PLDA-space transform (csrc/transform.hip), and the rule its
tests judge the device by.  NumPy only; nothing here restates the device's formula.

THE DEFINITION (Plda::TransformIvector), per row x with count n:
    t = T (x - mean)        w_d = 1 / (psi_d + 1/n)        s = sum_d t_d^2 w_d        out = sqrt(Dout / s) t
evaluated in np.longdouble (64-bit significand) from the fp64 inputs: `model`.

THE FORWARD BOUND, first order, for a device that evaluates fl(T x) + fl(-T mean) in fp64 in ANY summation order, u = 2^-53:
    E_o   = (Din + 2) u sum_k |T_ok| (|x_k| + |mean_k|) + u |t_o|      each product sum of Din terms carries at most Din u of its
                                                                     absolute sum, the two more are the offset's own rounding and
                                                                     the addition; u |t_o| is the rounding of the result
    rel_s = (sum_d 2 |t_d| E_d w_d) / s + (Dout + 4) u                 the sum of Dout positive terms in any order, squares and
                                                                     weights rounded
    B_o   = f E_o + |out_o| (rel_s / 2 + 4 u)                          f = sqrt(Dout / s); 4 u: the refined rsq, sqrt(Dout), two products
It is derived, not measured, and it grows with |mean|: the honest statement of what the offset form costs.  A row whose
rel_s exceeds VACUOUS is excluded (the first-order bound says nothing there); the tests assert that none is, for their inputs.

THE NORMALISER RESIDUAL  rho = | sum_d out_d^2 w_d / Dout - 1 |  on the DEVICE's own output, in longdouble with longdouble w,
bounded by (Dout + 24) u: Dout u for the sum of Dout terms, and 24 u for everything per element -- the factor enters squared
(2 x 4 u for the refined rsq, 2 x 3 u for sqrt(Dout) and the two products), the weights once (3 u for the refined reciprocal,
2 u for psi + 1/n), the squares and their products the rest.  The constants rest on the kernel's claim "hardware estimate +
two Newton steps: full precision", which is what the residual checks.  rho does not see the GEMM's error at all, and it is
sharp at small Dout.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
VACUOUS = 1e-3
POOL = 61            # prime: the copies of a pool entry land on every position mod 16, 64 and 128


def longdouble_is_extended():
    return np.finfo(LD).nmant >= 63


def make_model(rng, din, dout, mean_size=1.0):
    """(mean, T [dout, din], psi): rows of an orthogonal matrix scaled by 0.5 .. 1.5, psi descending in (0.01, 3.01); the mean is
    uniform in [0, 1) times mean_size (0: exactly zero)."""
    q, _ = np.linalg.qr(rng.standard_normal((din, din)))
    T = np.ascontiguousarray((q * (0.5 + rng.random(din))[:, None])[:dout])
    mean = rng.random(din) * mean_size if mean_size else np.zeros(din)
    psi = np.sort(rng.random(dout) * 3.0 + 0.01)[::-1].copy()
    return mean, T, psi


def _counts(n, r, dtype):
    n = np.asarray(n)
    return (np.full(r, n, dtype) if n.ndim == 0 else n.astype(dtype))[:, None]


def model(T, mean, psi, x, n, dtype=LD, dx=None):
    """The definition and its bound for rows x [R, Din] with counts n (a scalar or [R]) -> dict of [R, Dout] arrays `out`, `B`
    and [R] arrays `rel_s`, `s`, all in `dtype` (np.float64: the same formulas in fp64, for bounds over many rows; see
    bound_fp64).  x may be longdouble (rows that are themselves results, such as group means): dx [R, Din] then bounds the
    absolute error of the fp64 rows the device works on, and enters E through |T|."""
    T, mean, psi = (np.asarray(a, np.float64).astype(dtype) for a in (T, mean, psi))
    x = np.asarray(x).astype(dtype)
    dout, din = T.shape
    r = x.shape[0]
    u = dtype(U)
    t = (x - mean) @ T.T
    w = 1 / (psi[None, :] + 1 / _counts(n, r, dtype))
    s = (t * t * w).sum(1)
    with np.errstate(all="ignore"):
        f = np.sqrt(dout / s)
        out = f[:, None] * t
        E = (din + 2) * u * ((np.abs(x) + np.abs(mean)[None, :]) @ np.abs(T).T) + u * np.abs(t)
        if dx is not None:
            E = E + np.asarray(dx).astype(dtype) @ np.abs(T).T
        rel_s = (2 * np.abs(t) * E * w).sum(1) / s + (dout + 4) * u
        B = f[:, None] * E + np.abs(out) * (rel_s / 2 + 4 * u)[:, None]
    return dict(out=out, B=B, rel_s=rel_s, s=s, t=t, w=w)


def rho(out, psi, n):
    """| sum_d out_d^2 w_d / Dout - 1 | per row of `out` (the device's), in longdouble."""
    o = np.asarray(out, np.float64).astype(LD)
    w = 1 / (np.asarray(psi, np.float64).astype(LD)[None, :] + 1 / _counts(n, o.shape[0], LD))
    return np.abs((o * o * w).sum(1) / o.shape[1] - 1)


def rho_bound(dout):
    return (dout + 24) * U


def offset_form(T, mean, psi, x, n, fault=None, n_uniform=3):
    """A NumPy fp64 evaluation of the offset form fl(T x) + fl(-T mean), the device's arithmetic in another summation order --
    and, with `fault`, one of the planted faults the rule must reject:
        "kstep"    the last 4-wide k-step of the contraction dropped (a ragged Din's last stage)
        "neighbour" 1/n taken from the neighbouring row
        "offset16" the offset left out from column 16 onwards
        "f"        the factor off by a relative 3e-14 (one Newton step short of full precision)
        "weight"   one weight w_d taken with the uniform count `n_uniform` instead of the row's"""
    T, mean, psi, x = (np.asarray(a, np.float64) for a in (T, mean, psi, x))
    dout, din = T.shape
    r = x.shape[0]
    offset = -(T @ mean)
    xs = x
    if fault == "kstep":
        xs = x.copy()
        xs[:, (din - 1) // 4 * 4:] = 0.0
    if fault == "offset16":
        offset = offset.copy()
        offset[16:] = 0.0
    nn = _counts(n, r, np.float64)
    if fault == "neighbour":
        nn = np.roll(nn, 1, axis=0)
    t = xs @ T.T + offset[None, :]
    w = 1.0 / (psi[None, :] + 1.0 / nn) * np.ones((r, 1))
    if fault == "weight":
        w[:, dout // 2] = 1.0 / (psi[dout // 2] + 1.0 / n_uniform)
    s = (t * t * w).sum(1)
    f = np.sqrt(dout / s)
    if fault == "f":
        f = f * (1.0 + 3e-14)
    return f[:, None] * t


def deviation(got, ref, rows=None):
    """|got - ref["out"]| / ref["B"] per element (rows: the entries of `ref` the rows of `got` correspond to), in longdouble."""
    out, B = (ref["out"], ref["B"]) if rows is None else (ref["out"][rows], ref["B"][rows])
    return np.abs(np.asarray(got, np.float64).astype(out.dtype) - out) / B


def judge(got, ref, psi, n, rows=None):
    """The figures of the rule, no assertion: {"dev": the largest |got - out| / B, "rho": the largest residual in units of u,
    "rel_s": the largest rel_s of the rows}."""
    rel_s = ref["rel_s"] if rows is None else ref["rel_s"][rows]
    return {"dev": float(np.max(deviation(got, ref, rows))), "rho": float(np.max(rho(got, psi, n)) / U), "rel_s": float(np.max(rel_s))}


def assert_well_posed(ref, what=""):
    """no row is excluded: asserted on the model's numbers before the device runs"""
    assert np.isfinite(ref["out"].astype(np.float64)).all() and (ref["s"] > 0).all(), "%s: a row without a direction" % what
    assert float(ref["rel_s"].max()) <= VACUOUS, "%s: rel_s = %.3g makes the bound vacuous" % (what, float(ref["rel_s"].max()))


def assert_rule(got, ref, psi, n, what="", rows=None):
    """THE RULE: every element within B (no factor: B holds for any summation order), every row's normaliser residual within
    (Dout + 24) u.  -> judge()'s figures."""
    got = np.asarray(got, np.float64)
    fig = judge(got, ref, psi, n, rows)
    assert np.isfinite(got).all(), "%s: %d non-finite elements" % (what, int((~np.isfinite(got)).sum()))
    assert fig["rel_s"] <= VACUOUS, "%s: rel_s = %.3g makes the bound vacuous" % (what, fig["rel_s"])
    assert fig["dev"] <= 1.0, "%s: an element is %.3g of its bound B away from the longdouble model" % (what, fig["dev"])
    assert fig["rho"] * U <= rho_bound(got.shape[1]), "%s: normaliser residual %.1f u > (Dout + 24) u = %d u" % (what, fig["rho"], got.shape[1] + 24)
    return fig


def bound_fp64(T, mean, psi, x, n):
    """`out` and `B` evaluated in fp64 for many rows -> (out, B).  For rules of the form |device - NumPy| <= 2 B: the device and a
    NumPy fp64 evaluation of the offset form are each within B of the definition.  The fp64 evaluation of B itself is a sum of
    non-negative terms, good to a relative (Din + Dout) u < 1e-12; the callers multiply by 1 + 1e-9."""
    m = model(T, mean, psi, x, n, dtype=np.float64)
    return m["out"], m["B"] * (1.0 + 1e-9), m["rel_s"]


def assert_rule_many(got, T, mean, psi, x, n, what="", sample=48, also=(), no_looser_than=None):
    """The rule for MANY distinct rows, where a longdouble product of all of them would take minutes: every row against a NumPy
    fp64 evaluation of the offset form within 2 B (the device and NumPy are each within B of the definition; B evaluated in
    fp64), and a seeded sample of `sample` rows -- the first, the last and the rows `also` among them -- under assert_rule
    itself, residual included.  no_looser_than = (rtol, atol): the flat band an older test held these inputs to against such a
    NumPy evaluation; every element is held to the SMALLER of the two, so nothing is looser than it was.  (B itself is not
    below that band everywhere: at 33 017 x 520 its largest element is 1.2e-11, on a row with a small sum s, its median 2e-12.)"""
    got, x = np.asarray(got, np.float64), np.asarray(x, np.float64)
    r = x.shape[0]
    cnt = np.asarray(n)
    _, B, rel_s = bound_fp64(T, mean, psi, x, n)
    assert float(rel_s.max()) <= VACUOUS, "%s: rel_s = %.3g makes the bound vacuous" % (what, float(rel_s.max()))
    ref = offset_form(T, mean, psi, x, n)
    tol = 2.0 * B
    if no_looser_than is not None:
        tol = np.minimum(tol, no_looser_than[0] * np.abs(ref) + no_looser_than[1])
    err = np.abs(got - ref)
    assert np.isfinite(got).all() and (err <= tol).all(), "%s: %d elements beyond 2 B of the NumPy evaluation (worst %.3g of it)" % (
        what, int((~(err <= tol)).sum()), float((err / tol).max()))
    rows = np.unique(np.concatenate([np.random.default_rng(r).integers(0, r, sample), [0, r - 1], np.asarray(also, np.int64)]))
    rows = rows[(rows >= 0) & (rows < r)]
    sub_n = cnt if cnt.ndim == 0 else cnt[rows]
    return assert_rule(got[rows], model(T, mean, psi, x[rows], sub_n), psi, sub_n, what)


# ------------------------------------------------------------------------------------------- the pool and its spread
def pool_rows(rng, din, mean, counts=(1, 2, 3, 5, 8, 100), spread=1.0):
    """POOL distinct (row, n) entries around `mean`: rows mean + spread * N(0, 1), counts drawn from `counts` with every one of them
    present and neighbours that differ."""
    x = mean[None, :] + spread * rng.standard_normal((POOL, din))
    n = np.asarray(counts, np.int32)[np.arange(POOL) % len(counts)]
    return x, n[rng.permutation(POOL)].copy()


def spread_index(rng, r):
    """row i of a launch of r rows takes pool entry perm[i mod POOL] (perm seeded): copies of an entry sit POOL rows apart"""
    return rng.permutation(POOL)[np.arange(r) % POOL]


def launches(plan):
    """[(first row, end row, block rows)] of the launches of a plan (LibPlda.transform_plan)"""
    out = []
    if plan["main_rows"]:
        out.append((0, plan["main_rows"], plan["main_block"]))
    if plan["tail_rows"]:
        out.append((plan["main_rows"], plan["main_rows"] + plan["tail_rows"], plan["tail_block"]))
    return out


def shapes_of(plan):
    """the block shapes a plan runs, as the set of block rows per launch kind: {("main", 128), ("tail", 16), ...}"""
    s = set()
    if plan["main_rows"]:
        s.add(("main", plan["main_block"]))
    if plan["tail_rows"]:
        s.add(("tail", plan["tail_block"]))
    return s


def assert_copies_identical(got, idx, plan, what=""):
    """all copies of a pool entry inside one launch are bit-identical -> [(rows of got, pool entries)] one representative per
    (launch, entry), for the rule.  A position-dependent fault -- a clamped row, another row's count, a staging race -- shows here."""
    bits = np.ascontiguousarray(np.asarray(got, np.float64)).view(np.uint64)
    reps = []
    for lo, hi, _ in launches(plan):
        sub, part = idx[lo:hi], bits[lo:hi]
        first = np.full(POOL, -1, np.int64)
        order = np.arange(hi - lo)[::-1]
        first[sub[order]] = order                      # the first occurrence of every entry in this launch
        same = (part == part[first[sub]]).all(1)
        bad = np.nonzero(~same)[0]
        assert bad.size == 0, "%s: %d rows of the launch [%d, %d) differ in bits from the first copy of their pool entry (first: row %d)" % (
            what, bad.size, lo, hi, lo + int(bad[0]))
        present = np.nonzero(first >= 0)[0]
        reps.append((lo + first[present], present))
    return np.concatenate([a for a, _ in reps]), np.concatenate([b for _, b in reps])
