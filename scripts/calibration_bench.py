"""Score-calibration measurements (DESIGN.md "Score calibration"): whole calls between HIP events, warm-up, >= 5 timed
repetitions, medians.

  matrix  on an M x Nt trials matrix scored from random D-dimensional operands (speaker centres + noise, 20 utterances per speaker on both sides):
            time per calibration pass (plda_calib_pass_matrix_dev), passes and total time of a fit
            (plda_calib_fit_matrix_dev), time of the map (plda_affine_map_dev, in place), and with --operands the pass and
            the fit of the operand form (plda_score_calib_*_dev: the slabs are re-scored per pass), beside two yardsticks
            taken in the same run:
            (a) plda_eer_matrix_dev on the same matrix -- the floor any labelled pass over this matrix has shown;
            (b) the same record with stock torch fp64 elementwise operations over row slabs of <= 2 GiB of scores --
                what a user would write today.
  list    pass and fit of the list form on N scores (1 % targets), host arrays in, upload included.

usage: calibration_bench.py matrix M Nt D [--operands] [--only-pass] [--reps 5] [--out FILE.json]
       calibration_bench.py list N [--reps 5] [--out FILE.json]
One JSON document on stdout (and in --out).  The shader clock the box reports right after the timed loops is recorded with it."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _engine(D):
    import torch
    from plda_amd import MPlda
    eng = MPlda(0)
    rng = np.random.default_rng(D)
    q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    eng.set_model(rng.random(D), q * (1.0 + rng.random(D))[:, None], np.sort(rng.random(D) * 4.0 + 0.05)[::-1].copy())
    eng.set_stream(torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream)
    return eng


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
    """The record of one pass with stock torch operations (fp64, the overflow-free forms of the header), slab by slab."""
    import torch
    sums = torch.zeros((2, 6), dtype=torch.float64, device=S.device)
    counts = torch.zeros(4, dtype=torch.int64, device=S.device)
    for r0 in range(0, S.shape[0], rows):
        s = S[r0:r0 + rows].to(torch.float64)
        tgt = es[r0:r0 + rows, None] == ts[None, :]
        y = a * s + c
        e = torch.exp(-y.abs())
        l1p = torch.log1p(e)
        r = 1.0 / (1.0 + e)
        q = e * r
        w = q * r
        pos = y >= 0
        p = torch.where(pos, r, q)
        for k, (L, g) in enumerate(((y.clamp(min=0) + l1p, p), ((-y).clamp(min=0) + l1p, torch.where(pos, q, r)))):
            mask = tgt if k else ~tgt
            for j, term in enumerate((L, g, g * s, w, w * s, w * s * s)):
                sums[k, j] += (term * mask).sum()
        counts[0] += tgt.sum()
        counts[1] += (~tgt).sum()
        counts[2] += (tgt & (s < theta)).sum()
        counts[3] += (~tgt & (s >= theta)).sum()
    return sums, counts


def matrix(args):
    import torch
    from plda_amd import calibration as CB, eer
    dev = torch.device("cuda", 0)
    M, Nt, D = args.M, args.Nt, args.D
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    es, ts = torch.arange(M, device=dev) // 20, torch.arange(Nt, device=dev) // 20
    centres = torch.randn((max(M, Nt) // 20 + 1, D), dtype=torch.float64, device=dev, generator=g)      # real speaker structure
    U = centres[es] + torch.randn((M, D), dtype=torch.float64, device=dev, generator=g)
    V = centres[ts] + torch.randn((Nt, D), dtype=torch.float64, device=dev, generator=g)
    S = torch.empty((M, Nt), dtype=torch.float32, device=dev)
    eng = _engine(D)
    eng.score_matrix_dev(U.data_ptr(), None, 2, M, V.data_ptr(), Nt, S.data_ptr(), Nt)
    eng.synchronize()
    a, c, theta = 0.05, -0.4, 3.0
    ident = CB.Calibration(1.0, 0.0)                 # fma(1, s, 0) = s: the map's traffic and arithmetic, the matrix unchanged
    last = {}

    def one_pass():
        last["rec"] = CB.pass_from_matrix_dev(eng, S.data_ptr(), Nt, M, Nt, es.data_ptr(), ts.data_ptr(), a, c, theta)

    def fit():
        last["fit"] = CB.fit_from_matrix_dev(eng, S.data_ptr(), Nt, M, Nt, es.data_ptr(), ts.data_ptr())

    def amap():
        CB.apply_dev(eng, S.data_ptr(), Nt, M, Nt, ident)

    def eer_call():
        last["eer"] = eer.eer_from_matrix_dev(eng, S.data_ptr(), Nt, M, Nt, es.data_ptr(), ts.data_ptr())

    rows = max(1, min(M, (2 << 30) // 4 // Nt))

    def torch_call():
        last["torch"] = torch_record(S, es, ts, a, c, theta, rows)

    out = {"what": "plda_calib_pass_matrix_dev / plda_calib_fit_matrix_dev / plda_affine_map_dev", "M": M, "Nt": Nt, "D": D,
           "trials": M * Nt, "score_bytes": M * Nt * 4, "pass_point": [a, c, theta]}
    out["pass"] = _timed(one_pass, args.reps)
    if args.only_pass:                                # (under a counter collection: the pass alone)
        return out
    out["eer_matrix_same_matrix"] = _timed(eer_call, args.reps)
    out["torch_fp64_record_slabs_of_2GiB"] = dict(_timed(torch_call, args.reps, warmup=1), slab_rows=rows)
    out["pass_again"] = _timed(one_pass, args.reps)  # alternated: the spread between two windows of one code
    out["fit"] = _timed(fit, args.reps, warmup=1)
    f = last["fit"]
    out["fit_result"] = {"a": f.a, "b": f.b, "iterations": f.iterations, "passes": f.passes, "converged": f.converged,
                         "separable": f.separable, "cllr_before": f.cllr_before, "cllr_after": f.cllr_after}
    out["affine_map_in_place"] = _timed(amap, args.reps)
    tp = out["pass"]["median_ms"]
    out["pass_GBps_of_4_bytes_per_trial"] = M * Nt * 4 / (tp * 1e-3) / 1e9
    out["pass_ns_per_1000_trials"] = tp * 1e6 / (M * Nt) * 1e3
    out["pass_over_eer"] = tp / out["eer_matrix_same_matrix"]["median_ms"]
    out["torch_over_pass"] = out["torch_fp64_record_slabs_of_2GiB"]["median_ms"] / tp
    out["map_TBps_of_8_bytes_per_trial"] = M * Nt * 8 / (out["affine_map_in_place"]["median_ms"] * 1e-3) / 1e12
    sums, counts = last["torch"]
    rec = last["rec"]
    mine = np.array([[rec[n + "_n"] for n in CB.SUMS], [rec[n + "_t"] for n in CB.SUMS]])
    ref = sums.cpu().numpy()
    out["max_relative_difference_to_torch_record"] = float(np.max(np.abs(mine - ref) / np.maximum(np.abs(ref), 1e-300)))
    out["counts_equal_torch"] = [int(v) for v in counts.cpu().numpy()] == [rec["Np"], rec["Nn"], rec["miss"], rec["fa"]]
    if args.operands:
        def opass():
            CB.pass_from_operands_dev(eng, U.data_ptr(), None, 2, M, V.data_ptr(), Nt, es.data_ptr(), ts.data_ptr(), None, None, a, c, theta)

        def ofit():
            last["ofit"] = CB.fit_from_operands_dev(eng, U.data_ptr(), None, 2, M, V.data_ptr(), Nt, es.data_ptr(), ts.data_ptr())

        def gemm():
            eng.score_matrix_dev(U.data_ptr(), None, 2, M, V.data_ptr(), Nt, S.data_ptr(), Nt)
        out["operands_pass"] = _timed(opass, args.reps, warmup=1)
        out["operands_fit"] = dict(_timed(ofit, args.reps, warmup=1), passes=last["ofit"].passes)
        out["score_matrix_alone"] = _timed(gemm, args.reps, warmup=1)
    out["shader_clock_after"] = _clock()
    return out


def lists(args):
    from plda_amd import calibration as CB
    n = args.M
    rng = np.random.default_rng(4)
    npos = max(1, n // 100)
    pos = (2.0 + 2.0 * rng.standard_normal(npos)).astype(np.float32)
    neg = (-2.0 + 2.0 * rng.standard_normal(n - npos)).astype(np.float32)
    eng = _engine(32)
    last = {}

    def one_pass():
        CB.pass_from_lists(eng, pos, neg, 0.9, 0.1, 0.0)

    def fit():
        last["fit"] = CB.fit_from_lists(eng, pos, neg)
    out = {"what": "plda_calib_pass_lists / plda_calib_fit_lists (host arrays in: the upload is inside the call)", "N": n, "targets": npos}
    out["pass"] = _timed(one_pass, args.reps)
    out["fit"] = _timed(fit, args.reps, warmup=1)
    f = last["fit"]
    out["fit_result"] = {"a": f.a, "b": f.b, "iterations": f.iterations, "passes": f.passes, "converged": f.converged}
    out["pass_again"] = _timed(one_pass, args.reps)
    out["shader_clock_after"] = _clock()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["matrix", "list"])
    ap.add_argument("M", type=int)
    ap.add_argument("Nt", type=int, nargs="?", default=0)
    ap.add_argument("D", type=int, nargs="?", default=64)
    ap.add_argument("--operands", action="store_true", help="matrix: also time the operand form (slabs re-scored per pass)")
    ap.add_argument("--only-pass", action="store_true", help="matrix: time the pass alone (for a run under rocprofv3 --pmc)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("calibration_bench.py: no GPU -- these are measurements, there is nothing to fall back to")
    res = matrix(args) if args.mode == "matrix" else lists(args)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
