"""Diarisation error rate measurements: whole calls between HIP events, warm-up, >= 5 timed
repetitions, medians; the shader clock the box reports right after the timed loops is recorded with them.

Seeded recordings as in scripts/ahc_bench.py, with about 10 planted reference speakers each; the hypotheses are the device
AHC's own labels at a score threshold of 0, the sweep runs over its full merge record at Q = 32 thresholds.
Shapes: R = 2 000 recordings of N = 100 segments, R = 200 of N = 1 000 and R = 16 of N = 4 096.
Timed separately:
  der      plda_der_dev on labels and durations in HBM (count kernel, the call's wait, solve kernels, the final wait)
  sweep    plda_der_sweep_dev on the merge record in HBM, Q = 32
The yardstick is what a user does without the library, on this box's host, one thread, labels already in host memory: the
NumPy confusion matrix plus scipy.optimize.linear_sum_assignment (where scipy is missing: the tests' model, tests/der_model.py);
for the sweep Q x (diarize.cut + that), timed on at most `--host-recordings` recordings and scaled to R.  The counts of both
sides are compared for equality and the result is recorded.

No ratio is fixed in advance: the document records, it does not judge.

usage: der_bench.py [--reps 5] [--shapes 2000x100,200x1000,16x4096] [--q 32] [--host-recordings 16] [--out FILE.json]
       (default: profiles/der_<R>x<N>.json per shape)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from ahc_bench import D, _clock, _timed, synthetic_model  # noqa: E402

SPEAKERS = 10


def recordings(r, n, psi, seed):
    """segment vectors [r * n, D] in the model's space, the planted speaker of each (about 10 per recording, unequal
    counts, a tenth of the segments reference non-speech) and a duration in ticks"""
    rng = np.random.default_rng(seed)
    vecs = np.empty((r * n, D))
    ref = np.empty(r * n, np.int32)
    for q in range(r):
        k = min(n, int(rng.integers(SPEAKERS - 2, SPEAKERS + 3)))
        w = rng.random(k) ** 2 + 0.05
        g = rng.choice(k, size=n, p=w / w.sum())
        centres = rng.standard_normal((k, D)) * np.sqrt(psi)
        vecs[q * n:(q + 1) * n] = centres[g] + rng.standard_normal((n, D))
        ref[q * n:(q + 1) * n] = g
    ref[rng.random(r * n) < 0.1] = -1
    return vecs, ref, rng.integers(50, 300, r * n).astype(np.int32)


def host_solver():
    try:
        from scipy.optimize import linear_sum_assignment

        def solve(C):
            rows, cols = linear_sum_assignment(C, maximize=True)
            return int(C[rows, cols].sum())
        return solve, "scipy.optimize.linear_sum_assignment %s" % __import__("scipy").__version__
    except ImportError:
        import der_model
        return (lambda C: der_model.assign(C)[0]), "tests/der_model.py assign"


def host_counts(ref, hyp, dur, solve):
    """the NumPy confusion matrix and the assignment of ONE recording -> [speech, miss, fa, confusion]"""
    rs, hs = ref >= 0, hyp >= 0
    both = rs & hs
    _, ri = np.unique(ref[both], return_inverse=True)
    _, hi = np.unique(hyp[both], return_inverse=True)
    correct = 0
    if both.any():
        C = np.zeros((ri.max() + 1, hi.max() + 1), np.int64)
        np.add.at(C, (ri, hi), dur[both])
        correct = solve(C)
    return [int(dur[rs].sum()), int(dur[rs & ~hs].sum()), int(dur[~rs & hs].sum()), int(dur[both].sum()) - correct]


def measure(r, n, reps, nq, host_recs):
    import torch
    from plda_amd import MPlda, der, diarize
    dev = torch.device("cuda", 0)
    mean, T, psi = synthetic_model(D, 15)
    eng = MPlda(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    eng.set_model(mean, T, psi)
    vecs, ref, dur = recordings(r, n, psi, 1000 * r + n)
    offsets = diarize.offsets_of([n] * r)
    hyp, ncl = diarize.ahc_vectors(eng, vecs, offsets, 0.0, None)
    _, _, merges = diarize.ahc_vectors(eng, vecs, offsets, None, 1, return_merges=True)
    cost = merges[2][np.isfinite(merges[2])]
    thresholds = np.ascontiguousarray(-np.quantile(cost, np.linspace(0.5, 0.999, nq)))
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         (("ref", ref), ("hyp", hyp), ("dur", dur), ("ma", merges[0]), ("mb", merges[1]), ("mc", merges[2]))}
    counts = torch.empty((r, 4), dtype=torch.int64, device=dev)
    mp = torch.empty((r, 64), dtype=torch.int32, device=dev)
    scounts = torch.empty((nq, r, 4), dtype=torch.int64, device=dev)
    sncl = torch.empty((nq, r), dtype=torch.int32, device=dev)

    def f_der():
        eng.der_dev(d["ref"].data_ptr(), d["hyp"].data_ptr(), d["dur"].data_ptr(), offsets, counts.data_ptr(), mp.data_ptr())

    def f_sweep():
        eng.der_sweep_dev(d["ma"].data_ptr(), d["mb"].data_ptr(), d["mc"].data_ptr(), offsets, d["ref"].data_ptr(), d["dur"].data_ptr(),
                          thresholds, None, scounts.data_ptr(), sncl.data_ptr())

    res = {"what": "diarisation error rate: optimal speaker mapping; sweep of one merge record",
           "R": r, "N": n, "Q": nq, "segments": r * n, "reference_speakers": SPEAKERS,
           "hypothesis_speakers": {"min": int(ncl.min()), "median": float(np.median(ncl)), "max": int(ncl.max())},
           "class_at_median": der.plan(eng, SPEAKERS, int(np.median(ncl)))}
    res["der"] = _timed(f_der, reps)
    res["sweep"] = _timed(f_sweep, reps)
    torch.cuda.synchronize()
    res["clock_after"] = _clock()
    dc, sc, sk = counts.cpu().numpy(), scounts.cpu().numpy(), sncl.cpu().numpy()
    res["pooled_der_at_threshold_0"] = der.pooled(dc)
    res["sweep_pooled_der"] = {"best_q": der.best_index(sc), "min": float(np.nanmin([der.pooled(c) for c in sc])),
                               "clusters_median_first_last": [float(np.median(sk[0])), float(np.median(sk[-1]))]}

    solve, name = host_solver()
    hr = min(r, host_recs)
    t0 = time.perf_counter()
    hc = [host_counts(ref[q * n:(q + 1) * n], hyp[q * n:(q + 1) * n], dur[q * n:(q + 1) * n], solve) for q in range(hr)]
    t_der = time.perf_counter() - t0
    sub_off = offsets[:hr + 1]
    sub_m = tuple(a[:int(sub_off[-1]) - hr] for a in merges)
    t0 = time.perf_counter()
    hs = []
    for thr in thresholds:
        labels, _ = diarize.cut(sub_m, sub_off, float(thr))
        hs.append([host_counts(ref[q * n:(q + 1) * n], labels[q * n:(q + 1) * n], dur[q * n:(q + 1) * n], solve) for q in range(hr)])
    t_sweep = time.perf_counter() - t0
    res["host_baseline"] = {"solver": name, "threads": 1, "recordings_timed": hr, "der_ms_scaled_to_R": 1e3 * t_der * r / hr,
                   "sweep_ms_scaled_to_R": 1e3 * t_sweep * r / hr,
                   "der_equals_device": bool(np.array_equal(np.asarray(hc), dc[:hr])),
                   "sweep_equals_device": bool(np.array_equal(np.asarray(hs), sc[:, :hr]))}
    res["host_over_device"] = {"der": res["host_baseline"]["der_ms_scaled_to_R"] / res["der"]["median_ms"],
                               "sweep": res["host_baseline"]["sweep_ms_scaled_to_R"] / res["sweep"]["median_ms"]}
    del eng
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="2000x100,200x1000,16x4096")
    ap.add_argument("--q", type=int, default=32)
    ap.add_argument("--host-recordings", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("der_bench.py: no GPU -- these are measurements, there is nothing to fall back to")
    for shape in args.shapes.split(","):
        r, n = (int(v) for v in shape.split("x"))
        res = measure(r, n, args.reps, args.q, args.host_recordings)
        path = args.out or os.path.join(ROOT, "profiles", "der_%dx%d.json" % (r, n))
        if args.out and len(args.shapes.split(",")) > 1:
            path = "%s.%dx%d.json" % (os.path.splitext(args.out)[0], r, n)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({k: res[k] for k in res if k != "what"}), flush=True)


if __name__ == "__main__":
    main()
