"""AS-norm measurements: whole calls between HIP events, warm-up, >= 5 timed repetitions, medians.

  stats   plda_cohort_stats_dev on R x Nc (D, K) against
            (a) the floor: plda_score_matrix_dev alone on the same slabs (the scores must be produced) -> select overhead
                = t_stats / t_gemm - 1;
            (b) what a caller could do before: plda_score_matrix_dev into a slab + torch.topk + moments in torch, same slabs;
          and, with --slab-rows a,b,c, the call itself over slab heights (PLDA_SNORM_SLAB_ROWS; fresh handles).
  apply   plda_score_matrix_snorm_dev (both sides) against plda_score_matrix_dev with z-norm statistics on M x Nt: the ratio,
          and the post-pass alone (snorm minus the plain matrix) against its floor of one read + one write of the matrix.

usage: asnorm_bench.py stats R Nc D K [--slab-rows 256,1024] [--only-call] [--reps 5] [--out FILE.json]
       asnorm_bench.py apply M Nt D [--reps 5] [--out FILE.json]
One JSON document on stdout (and in --out).  The shader clock the box reports right after the timed loops is recorded with it."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _engine(D, slab_rows=None):
    import torch
    from plda_amd import MPlda
    if slab_rows:
        os.environ["PLDA_SNORM_SLAB_ROWS"] = str(slab_rows)
    else:
        os.environ.pop("PLDA_SNORM_SLAB_ROWS", None)
    eng = MPlda(0)
    os.environ.pop("PLDA_SNORM_SLAB_ROWS", None)
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


def _default_slab_rows(R, Nc):
    ld = (Nc + 3) // 4 * 4
    return min(max(256, ((2 << 30) // 4 // ld) // 256 * 256), (4 << 30) // 4 // ld, R)


def stats(args):
    import torch
    dev = torch.device("cuda", 0)
    R, Nc, D, K = args.R, args.Nc, args.D, args.K
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    X = torch.randn((R, D), dtype=torch.float64, device=dev, generator=g)
    Cv = torch.randn((Nc, D), dtype=torch.float64, device=dev, generator=g)
    res = torch.empty((2, R), dtype=torch.float64, device=dev)
    eng = _engine(D)
    rows = _default_slab_rows(R, Nc)
    slab = torch.empty((rows, Nc), dtype=torch.float32, device=dev)
    base = torch.empty((2, R), dtype=torch.float64, device=dev)

    def call(e=eng):
        e.cohort_stats_dev(X.data_ptr(), None, 1, R, Cv.data_ptr(), Nc, K, res[0].data_ptr(), res[1].data_ptr())

    def gemm_only():
        for r0 in range(0, R, rows):
            m = min(rows, R - r0)
            eng.score_matrix_dev(X[r0:r0 + m].data_ptr(), None, 1, m, Cv.data_ptr(), Nc, slab.data_ptr(), Nc)

    def gemm_topk():
        for r0 in range(0, R, rows):
            m = min(rows, R - r0)
            eng.score_matrix_dev(X[r0:r0 + m].data_ptr(), None, 1, m, Cv.data_ptr(), Nc, slab.data_ptr(), Nc)
            top = torch.topk(slab[:m], K, dim=1).values.to(torch.float64)
            base[0, r0:r0 + m] = top.mean(dim=1)
            base[1, r0:r0 + m] = top.std(dim=1, unbiased=False)

    out = {"what": "plda_cohort_stats_dev", "R": R, "Nc": Nc, "D": D, "K": K, "slab_rows": rows,
           "scores": R * Nc, "score_bytes": R * Nc * 4}
    out["cohort_stats"] = _timed(call, args.reps)
    if args.only_call:                     # (under a counter collection: the call alone)
        return out
    out["gemm_only_same_slabs"] = _timed(gemm_only, args.reps)
    out["gemm_plus_torch_topk_same_slabs"] = _timed(gemm_topk, args.reps)
    out["cohort_stats_again"] = _timed(call, args.reps)                  # alternated: the spread between two windows of one code
    t, tg, tb = out["cohort_stats"]["median_ms"], out["gemm_only_same_slabs"]["median_ms"], out["gemm_plus_torch_topk_same_slabs"]["median_ms"]
    out["select_overhead"] = t / tg - 1.0
    out["speedup_over_torch_topk"] = tb / t
    out["select_ms"] = t - tg
    out["select_GBps_per_read_of_the_scores"] = R * Nc * 4 / ((t - tg) * 1e-3) / 1e9 if t > tg else None
    call()
    torch.cuda.synchronize()
    d = (res - base).abs().max(dim=1).values.cpu().numpy()
    out["max_abs_difference_to_torch_topk"] = {"mean": float(d[0]), "std": float(d[1])}
    if args.slab_rows:
        sweep = {}
        for sr in [int(s) for s in args.slab_rows.split(",")]:
            e2 = _engine(D, sr)
            sweep[str(sr)] = _timed(lambda e2=e2: call(e2), args.reps)
            e2.synchronize()
            del e2
        out["slab_rows_sweep"] = sweep
    out["shader_clock_after"] = _clock()
    return out


def apply(args):
    import torch
    dev = torch.device("cuda", 0)
    M, Nt, D = args.R, args.Nc, args.D
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    U = torch.randn((M, D), dtype=torch.float64, device=dev, generator=g)
    V = torch.randn((Nt, D), dtype=torch.float64, device=dev, generator=g)
    em, es = torch.randn(M, dtype=torch.float64, device=dev, generator=g), torch.rand(M, dtype=torch.float64, device=dev, generator=g) + 0.5
    tm, ts = torch.randn(Nt, dtype=torch.float64, device=dev, generator=g), torch.rand(Nt, dtype=torch.float64, device=dev, generator=g) + 0.5
    outm = torch.empty((M, Nt), dtype=torch.float32, device=dev)
    eng = _engine(D)

    def plain():
        eng.score_matrix_dev(U.data_ptr(), None, 1, M, V.data_ptr(), Nt, outm.data_ptr(), Nt)

    def znorm():
        eng.score_matrix_dev(U.data_ptr(), None, 1, M, V.data_ptr(), Nt, outm.data_ptr(), Nt, dzmean=em.data_ptr(), dzstd=es.data_ptr())

    def snorm():
        eng.score_matrix_snorm_dev(U.data_ptr(), None, 1, M, V.data_ptr(), Nt, outm.data_ptr(), Nt, em.data_ptr(), es.data_ptr(),
                                   tm.data_ptr(), ts.data_ptr())

    out = {"what": "plda_score_matrix_snorm_dev", "M": M, "Nt": Nt, "D": D, "trials": M * Nt}
    out["score_matrix_plain"] = _timed(plain, args.reps)
    out["score_matrix_znorm"] = _timed(znorm, args.reps)
    out["score_matrix_snorm"] = _timed(snorm, args.reps)
    out["score_matrix_znorm_again"] = _timed(znorm, args.reps)
    ts_, tz, tp = out["score_matrix_snorm"]["median_ms"], out["score_matrix_znorm"]["median_ms"], out["score_matrix_plain"]["median_ms"]
    out["snorm_over_znorm"] = ts_ / tz
    out["post_pass_ms"] = ts_ - tp
    out["post_pass_TBps_of_8_bytes_per_trial"] = M * Nt * 8 / ((ts_ - tp) * 1e-3) / 1e12 if ts_ > tp else None
    out["shader_clock_after"] = _clock()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["stats", "apply"])
    ap.add_argument("R", type=int)
    ap.add_argument("Nc", type=int)
    ap.add_argument("D", type=int)
    ap.add_argument("K", type=int, nargs="?", default=300)
    ap.add_argument("--slab-rows", default="")
    ap.add_argument("--only-call", action="store_true", help="stats: time the call alone (for a run under rocprofv3 --pmc)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("asnorm_bench.py: no GPU -- these are measurements, there is nothing to fall back to")
    res = stats(args) if args.mode == "stats" else apply(args)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
