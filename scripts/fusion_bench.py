"""Score-fusion measurements: whole calls between HIP events, warm-up, >= 5 timed repetitions,
medians.

On K trials matrices [M, Nt] (a common part with 20 utterances per speaker on both sides, targets higher, plus each system's
own noise and units) it times one fusion pass (plda_fusion_pass_matrices_dev), one fit (plda_fusion_fit_matrices_dev) and the
map (plda_fusion_map_dev into a matrix of its own), beside two yardsticks taken in the same run:
  (a) K = 1 only: plda_calib_pass_matrix_dev on the same matrix at the same point -- the same per-element arithmetic;
  (b) the same record with stock torch fp64 elementwise operations over row slabs of <= 2 GiB of fp64 temporaries --
      what a user would write today (the baseline of scripts/calibration_bench.py).

The run FAILS (non-zero exit, after the document is written) if the exact counts differ from (b)'s, if a sum differs from
(b)'s by more than 1e-9 relative, or if the pass is not faster than (b) -- the requirement at 20 000 x 20 000, K = 3.

usage: fusion_bench.py M Nt K [--reps 5] [--only-pass] [--no-torch] [--out FILE.json]
One JSON document on stdout (and in --out).  The shader clock the box reports right after the timed loops is recorded with it."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, reps, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": reps}


def _clock():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln.lower()][:2]
    except Exception as ex:      # noqa: BLE001 -- the clock line is a note, not a measurement
        return ["not read: %s" % ex]


def torch_record(S, es, ts, a, c, theta, rows):
    """The record of one fusion pass with stock torch operations (fp64, the overflow-free forms of the header), slab by slab:
    per class L, G[K + 1], H[(K + 1)(K + 2) / 2], and the four counts."""
    import torch
    k = len(S)
    ne = 1 + (k + 1) + (k + 1) * (k + 2) // 2
    sums = torch.zeros((2, ne), dtype=torch.float64, device=S[0].device)
    counts = torch.zeros(4, dtype=torch.int64, device=S[0].device)
    for r0 in range(0, S[0].shape[0], rows):
        s = [x[r0:r0 + rows].to(torch.float64) for x in S]
        tgt = es[r0:r0 + rows, None] == ts[None, :]
        y = torch.full_like(s[0], c)
        for ak, sk in zip(a, s):
            y = y + float(ak) * sk
        e = torch.exp(-y.abs())
        l1p = torch.log1p(e)
        r = 1.0 / (1.0 + e)
        q = e * r
        w = q * r
        pos = y >= 0
        p = torch.where(pos, r, q)
        phi = [None] + s
        for cl, (L, g) in enumerate(((y.clamp(min=0) + l1p, p), ((-y).clamp(min=0) + l1p, torch.where(pos, q, r)))):
            mask = tgt if cl else ~tgt
            gm, wm = g * mask, w * mask
            sums[cl, 0] += (L * mask).sum()
            sums[cl, 1] += gm.sum()
            for j in range(1, k + 1):
                sums[cl, 1 + j] += (gm * phi[j]).sum()
            for j in range(k + 1):
                for i in range(j + 1):
                    t = wm if j == 0 else (wm * phi[j] if i == 0 else wm * phi[i] * phi[j])
                    sums[cl, k + 2 + j * (j + 1) // 2 + i] += t.sum()
        counts[0] += tgt.sum()
        counts[1] += (~tgt).sum()
        counts[2] += (tgt & (y < theta)).sum()
        counts[3] += (~tgt & (y >= theta)).sum()
    return sums, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("M", type=int)
    ap.add_argument("Nt", type=int)
    ap.add_argument("K", type=int)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-pass", action="store_true", help="time the pass alone (for a run under rocprofv3 --pmc)")
    ap.add_argument("--no-torch", action="store_true", help="skip yardstick (b)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("fusion_bench.py: no GPU -- these are measurements, there is nothing to fall back to")
    from plda_amd import MPlda, calibration as CB, fusion as FU
    dev = torch.device("cuda", 0)
    M, Nt, K = args.M, args.Nt, args.K
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    es, ts = torch.arange(M, device=dev) // 20, torch.arange(Nt, device=dev) // 20
    unit = [1.0, 150.0, 0.4, 1.0, 1.5, 0.7, 2.0, 1.2]
    shift = [0.0, 0.0, 0.0, -20.0, 0.0, 0.0, 0.0, 0.0]
    S = []
    rows_gen = max(1, min(M, (1 << 28) // Nt))
    for k in range(K):
        X = torch.empty((M, Nt), dtype=torch.float32, device=dev)
        gb = torch.Generator(device=dev)
        for r0 in range(0, M, rows_gen):              # the common part is regenerated from its seed for every system
            gb.manual_seed(1000 + r0)
            base = torch.randn((min(rows_gen, M - r0), Nt), dtype=torch.float32, device=dev, generator=gb) * 2.0 - 1.0
            base += 2.5 * (es[r0:r0 + rows_gen, None] == ts[None, :])
            base += 1.5 * torch.randn(base.shape, dtype=torch.float32, device=dev, generator=g)
            X[r0:r0 + rows_gen] = unit[k] * base + shift[k]
        S.append(X)
    out_m = torch.empty((M, Nt), dtype=torch.float32, device=dev)
    eng = MPlda(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    ptrs, lds = [x.data_ptr() for x in S], [Nt] * K
    a = np.array([0.15 / u for u in unit[:K]])
    c, theta = -0.4, 0.3
    last = {}

    def one_pass():
        last["rec"] = FU.pass_from_matrices_dev(eng, ptrs, lds, M, Nt, es.data_ptr(), ts.data_ptr(), a, c, theta)

    def fit():
        last["fit"] = FU.fit_from_matrices_dev(eng, ptrs, lds, M, Nt, es.data_ptr(), ts.data_ptr())

    def fmap():
        FU.apply_dev(eng, ptrs, lds, M, Nt, FU.Fusion(a, c), out_m.data_ptr(), Nt)

    def calib_pass():
        last["calib"] = CB.pass_from_matrix_dev(eng, ptrs[0], Nt, M, Nt, es.data_ptr(), ts.data_ptr(), float(a[0]), c, theta)

    ne = 1 + (K + 1) + (K + 1) * (K + 2) // 2
    out = {"what": "plda_fusion_pass_matrices_dev / plda_fusion_fit_matrices_dev / plda_fusion_map_dev", "M": M, "Nt": Nt, "K": K,
           "trials": M * Nt, "score_bytes": M * Nt * 4 * K, "sums_per_class": ne, "pass_point": [a.tolist(), c, theta]}
    out["pass"] = _timed(one_pass, args.reps)
    if not args.only_pass:
        if K == 1:
            out["calib_pass_same_matrix"] = _timed(calib_pass, args.reps)
            out["calib_pass_same_matrix_again"] = _timed(calib_pass, args.reps)     # the spread of two runs of (a)
        if not args.no_torch:
            rows = max(1, min(M, (2 << 30) // 8 // Nt))
            out["torch_fp64_record_slabs"] = dict(_timed(lambda: last.__setitem__("torch", torch_record(S, es, ts, a, c, theta, rows)),
                                                         max(2, args.reps // 2), warmup=1), slab_rows=rows)
        out["pass_again"] = _timed(one_pass, args.reps)
        out["fit"] = _timed(fit, max(2, args.reps // 2), warmup=1)
        f = last["fit"]
        out["fit_result"] = {"a": f.a.tolist(), "b": f.b, "iterations": f.iterations, "passes": f.passes, "converged": f.converged,
                             "separable": f.separable, "cllr_after": f.cllr_after}
        out["map"] = _timed(fmap, args.reps)
        tp = out["pass"]["median_ms"]
        out["pass_GBps_of_4K_bytes_per_trial"] = M * Nt * 4 * K / (tp * 1e-3) / 1e9
        out["pass_ps_per_trial"] = tp * 1e9 / (M * Nt)
        out["map_TBps_of_4K_plus_4_bytes_per_trial"] = M * Nt * 4 * (K + 1) / (out["map"]["median_ms"] * 1e-3) / 1e12
        if K == 1:
            out["pass_over_calib_pass"] = tp / out["calib_pass_same_matrix"]["median_ms"]
        if "torch" in last:
            out["torch_over_pass"] = out["torch_fp64_record_slabs"]["median_ms"] / tp
            sums, counts = last["torch"]
            rec = last["rec"]
            mine = np.array([[rec["L_" + cl]] + list(rec["G_" + cl]) + list(rec["H_" + cl]) for cl in ("n", "t")])
            ref = sums.cpu().numpy()
            out["max_relative_difference_to_torch_record"] = float(np.max(np.abs(mine - ref) / np.maximum(np.abs(ref), 1e-300)))
            out["counts_equal_torch"] = [int(v) for v in counts.cpu().numpy()] == [rec["Np"], rec["Nn"], rec["miss"], rec["fa"]]
    out["shader_clock_after"] = _clock()
    # what must hold, not only be printed: the counts are exact in both computations, and the pass beats the baseline
    failures = []
    if out.get("counts_equal_torch") is False:
        failures.append("the exact counts differ from the stock-torch record")
    if "max_relative_difference_to_torch_record" in out and not out["max_relative_difference_to_torch_record"] <= 1e-9:
        failures.append("a sum differs from the stock-torch record by %.3g relative" % out["max_relative_difference_to_torch_record"])
    if "torch_over_pass" in out and not out["torch_over_pass"] > 1.0:
        failures.append("the pass is not faster than the same record through stock torch (ratio %.3g)" % out["torch_over_pass"])
    out["failures"] = failures
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    if failures:
        sys.exit("fusion_bench.py: " + "; ".join(failures))


if __name__ == "__main__":
    main()
