"""NumPy model of the VBx resegmentation (include/plda_hip.h, "VBx resegmentation"; csrc/vbx.hip): the contract restated step by
step with the floating type as a parameter (np.float64, np.longdouble), the published log-domain form of the same iteration for
cross-checking, and the generator of the test recordings.  Not product code: tests/ and scripts/vbx_bench.py import it."""
import numpy as np

MAX_SPK = 64               # PLDA_VBX_MAX_SPK
LDS_DOUBLES = 19456        # the LDS class's limit in doubles of state (plda_vbx_plan out[2])

# (Fa, Fb, loop_prob) of the tests
PARAMS = {"default": (0.3, 17.0, 0.99), "mid": (0.4, 64.0, 0.65), "unit": (1.0, 1.0, 0.9)}


def state_doubles(t, s, d):
    """the per-recording state of csrc/vbx.hip in doubles: b, a, beta [T, S]; c, m, G [T]; alpha, invL [S, D | 1]; sqrt Phi, Phi"""
    return 3 * t * s + 3 * t + 2 * s * (d | 1) + 2 * d


def generate(t, d, k, s, seed):
    """One recording: Phi[d] = 30 exp(-4 d / D); k speakers ~ N(0, Phi); a sticky speaker sequence (stay probability 0.95);
    y = speaker + N(0, I); initial labels that over-split, (2 spk + t mod 2) mod s.  So that the recording HAS s initial
    speakers, the last segment takes label s - 1 where no segment has it (a label value without a segment is allowed, so the
    values between may stay empty).  -> (y [t, d], labels int32 [t], spk [t], phi [d])"""
    rng = np.random.default_rng(seed)
    phi = 30.0 * np.exp(-4.0 * np.arange(d) / d)
    means = rng.standard_normal((k, d)) * np.sqrt(phi)
    spk = np.empty(t, np.int64)
    cur = int(rng.integers(k))
    for i in range(t):
        if i and rng.random() >= 0.95:
            cur = int(rng.integers(k))
        spk[i] = cur
    y = means[spk] + rng.standard_normal((t, d))
    labels = ((2 * spk + np.arange(t) % 2) % s).astype(np.int32)
    if labels.max() < s - 1:
        labels[-1] = s - 1
    return y, labels, spk, phi


def first_member_labels(raw):
    """labels renumbered 0 .. k-1 by ascending smallest member -> (labels int32, k)"""
    raw = np.asarray(raw)
    order = {}
    out = np.empty(len(raw), np.int32)
    for i, v in enumerate(raw.tolist()):
        out[i] = order.setdefault(v, len(order))
    return out, len(order)


def _start(y, labels, phi, sigma, f):
    y, phi = np.asarray(y, f), np.asarray(phi, f)
    t, d = y.shape
    s = int(np.max(labels)) + 1
    two_pi = 8 * np.arctan(f(1))
    rho = y * np.sqrt(phi)
    g = -(np.sum(y * y, axis=1) + d * np.log(two_pi)) / 2
    es = np.exp(f(sigma))
    gamma = np.full((t, s), 1 / (es + (s - 1)), f)
    gamma[np.arange(t), np.asarray(labels)] = es / (es + (s - 1))
    return y, phi, rho, g, gamma, np.full(s, 1 / f(s), f)


def _emission(gamma, rho, phi, g, fa, fb):
    """steps 1 - 4 and the ELBO's model term"""
    fafb = fa / fb
    n = gamma.sum(axis=0)
    inv_l = 1 / (1 + fafb * n[:, None] * phi[None, :])
    alpha = fafb * inv_l * (gamma.T @ rho)
    lp = fa * (rho @ alpha.T - ((inv_l + alpha * alpha) @ phi)[None, :] / 2 + g[:, None])
    reg = fb / 2 * np.sum(np.log(inv_l) - inv_l - alpha * alpha + 1)
    return lp, reg


def _finish(gamma, pi, elbo, iters, max_iters, max_lp):
    labels, k = first_member_labels(np.argmax(gamma, axis=1))
    full = np.full(max_iters, np.nan, gamma.dtype)
    full[:iters] = elbo
    return {"labels": labels, "n_clusters": k, "gamma": gamma, "pi": pi, "elbo": full, "iters": iters, "max_lp": max_lp}


def run(y, labels, phi, fa=0.3, fb=17.0, loop_prob=0.99, init_smoothing=5.0, max_iters=40, epsilon=1e-4, dtype=np.float64):
    """The contract: the scaled forward-backward."""
    f = dtype
    y, phi, rho, g, gamma, pi = _start(y, labels, phi, init_smoothing, f)
    t, s = gamma.shape
    fa, fb, p = f(fa), f(fb), f(loop_prob)
    elbo, max_lp = [], 0.0
    for i in range(max_iters):
        lp, reg = _emission(gamma, rho, phi, g, fa, fb)
        max_lp = max(max_lp, float(np.max(np.abs(lp))))
        m = lp.max(axis=1)
        b = np.exp(lp - m[:, None])
        a, c, beta = np.empty((t, s), f), np.empty(t, f), np.empty((t, s), f)
        u = b[0] * pi
        c[0] = u.sum()
        a[0] = u / c[0]
        for j in range(1, t):
            u = b[j] * (p * a[j - 1] + (1 - p) * pi)
            c[j] = u.sum()
            a[j] = u / c[j]
        beta[t - 1] = 1
        for j in range(t - 2, -1, -1):
            w = b[j + 1] * beta[j + 1]
            beta[j] = (p * w + (1 - p) * np.sum(pi * w)) / c[j + 1]
        gamma = a * beta
        like = np.sum(np.log(c)) + np.sum(m)
        pin = gamma[0] + (1 - p) * pi * np.sum(b[1:] * beta[1:] / c[1:, None], axis=0)
        pi = pin / pin.sum()
        elbo.append(like + reg)
        if i >= 1 and elbo[i] - elbo[i - 1] < epsilon:
            break
    return _finish(gamma, pi, elbo, len(elbo), max_iters, max_lp)


def _lse(x, axis):
    m = np.max(x, axis=axis, keepdims=True)
    return np.squeeze(m, axis) + np.log(np.sum(np.exp(x - m), axis=axis))


def run_log(y, labels, phi, fa=0.3, fb=17.0, loop_prob=0.99, init_smoothing=5.0, max_iters=40, epsilon=1e-4, dtype=np.float64):
    """The published log-domain form (VBx.py of the paper's recipe: forward_backward on log tr, log pi): the cross-check.
    Where pi underflows it produces -inf - -inf; `finite` says whether every quantity stayed finite."""
    f = dtype
    y, phi, rho, g, gamma, pi = _start(y, labels, phi, init_smoothing, f)
    t, s = gamma.shape
    fa, fb, p = f(fa), f(fb), f(loop_prob)
    elbo, finite = [], True
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(max_iters):
            lp, reg = _emission(gamma, rho, phi, g, fa, fb)
            ltr = np.log(p * np.eye(s, dtype=f) + (1 - p) * pi[None, :])
            lf, lb = np.empty((t, s), f), np.zeros((t, s), f)
            lf[0] = lp[0] + np.log(pi)
            for j in range(1, t):
                lf[j] = lp[j] + _lse(lf[j - 1][:, None] + ltr, 0)
            for j in range(t - 2, -1, -1):
                lb[j] = _lse(ltr + (lp[j + 1] + lb[j + 1])[None, :], 1)
            tll = _lse(lf[t - 1], 0)
            gamma = np.exp(lf + lb - tll)
            pin = gamma[0] + (1 - p) * pi * np.sum(np.exp(_lse(lf[:-1], 1)[:, None] + lp[1:] + lb[1:] - tll), axis=0)
            pi = pin / pin.sum()
            elbo.append(tll + reg)
            finite = finite and bool(np.isfinite(gamma).all() and np.isfinite(pi).all() and np.isfinite(elbo[-1]))
            if not finite or (i >= 1 and elbo[i] - elbo[i - 1] < epsilon):
                break
    out = _finish(gamma, pi, elbo, len(elbo), max_iters, 0.0)
    out["finite"] = finite
    return out


def margin(gamma):
    """the smallest top-two margin of gamma over the rows (inf for one speaker)"""
    if gamma.shape[1] < 2:
        return np.inf
    top = np.sort(np.asarray(gamma, np.float64), axis=1)
    return float(np.min(top[:, -1] - top[:, -2]))


def deviation(a, b):
    """(max |gamma_a - gamma_b|, max |pi_a - pi_b|, max relative ELBO difference over the iterations both ran)"""
    n = min(a["iters"], b["iters"])
    ea, eb = np.asarray(a["elbo"][:n], np.longdouble), np.asarray(b["elbo"][:n], np.longdouble)
    return (float(np.max(np.abs(np.asarray(a["gamma"], np.longdouble) - b["gamma"]))),
            float(np.max(np.abs(np.asarray(a["pi"], np.longdouble) - b["pi"]))),
            float(np.max(np.abs(ea - eb) / np.abs(eb))))


# ---- the cases of tests/test_gpu_vbx.py and the conditions tests/test_vbx_model.py asserts for them
ITERS = 20                 # the fixed number of iterations of the parity runs (epsilon = -inf)


def lds_boundary(d=16, s=8):
    """(largest T of the LDS class, smallest of the HBM class) at (d, s)"""
    t = 1
    while state_doubles(t + 1, s, d) <= LDS_DOUBLES:
        t += 1
    return t, t + 1


def cases():
    """name -> (T, D, K, S, parameter set).  The first two parameter sets collapse T <= 65 at D <= 16 to one speaker: those
    cases run with (1, 1, 0.9)."""
    lo, hi = lds_boundary()
    shapes = [(1, 4, 1, 1), (1, 4, 1, 2), (2, 4, 1, 1), (40, 8, 2, 3), (64, 16, 3, 33), (65, 16, 3, 64), (130, 7, 3, 5), (200, 33, 3, 6),
              (257, 130, 4, 12), (300, 64, 4, 10), (600, 48, 5, 16), (lo, 16, 4, 8), (hi, 16, 4, 8), (4096, 32, 4, 8)]
    out = {}
    for q, (t, d, k, s) in enumerate(shapes):
        small = t <= 65 and d <= 16
        out["%dx%dx%dx%d" % (t, d, k, s)] = (t, d, k, s, "unit" if small else ("default", "mid")[q % 2])
    return out


_CACHE = {}


def reference(name):
    """the case's recording and its fp64 and longdouble runs of ITERS iterations, computed once and left unchanged"""
    if name not in _CACHE:
        t, d, k, s, pset = cases()[name]
        y, labels, spk, phi = generate(t, d, k, s, 1000 + 7 * t + d)
        for a in (y, labels, spk, phi):
            a.setflags(write=False)
        fa, fb, p = PARAMS[pset]
        kw = dict(fa=fa, fb=fb, loop_prob=p, max_iters=ITERS, epsilon=-np.inf)
        _CACHE[name] = {"y": y, "labels": labels, "spk": spk, "phi": phi, "params": (fa, fb, p),
                        "f64": run(y, labels, phi, dtype=np.float64, **kw), "ld": run(y, labels, phi, dtype=np.longdouble, **kw)}
    return _CACHE[name]


def stop_epsilon(ref):
    """An epsilon at which the stop decision cannot hinge on rounding: the geometric mean of the first two successive
    improvements of the fp64 run that differ by at least 4x (every earlier improvement at least the larger of the two)
    -> (epsilon, the fp64 run with it)"""
    imp = np.diff(np.asarray(ref["f64"]["elbo"], np.float64))
    for i in range(len(imp) - 1):
        if imp[i + 1] > 0 and imp[i] >= 4 * imp[i + 1] and (imp[:i] >= imp[i]).all():
            eps = float(np.sqrt(imp[i] * imp[i + 1]))
            fa, fb, p = ref["params"]
            return eps, run(ref["y"], ref["labels"], ref["phi"], fa, fb, p, max_iters=ITERS, epsilon=eps)
    raise AssertionError("no two successive improvements 4x apart")


STOP_CASES = sorted(n for n, c in cases().items() if c[2] >= 2)      # every case with more than one planted speaker
