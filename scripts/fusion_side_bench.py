"""Quality-aware calibration measurements: the side instantiations of csrc/fusion.hip against its
matrix kernels on MATERIALISED sides -- the same library, the same process, the same trials.

Method: every arm is warmed first, then the two arms of a pair ALTERNATE (A B A B ...) between HIP events in one process, so
that clock drift and whatever else moves during the run lands on both; per arm the median, minimum and maximum, and per pair
the ratio of the medians next to each arm's own spread (max / min) -- a ratio inside the spread is no difference.

Pairs at M x Nt (default 20 000 x 20 000), one system and Q sides against K = 1 + Q matrices:
  pass  (1, 3) against the matrix pass at K = 4;   pass (1, 7) against K = 8;
  map   (1, 3) against the matrix map at K = 4;    map  (1, 7) against K = 8;
  fit   (1, 3) against the matrix fit at K = 4 (the results must be the same bytes).
With --operands M Nt: the operand-form fit (this model's own score re-scored slab by slab, Q = 3, no matrix held) alone.
Bytes moved per trial are computed from the shapes: a matrix arm reads 4 T (pass) or reads 4 T and writes 4 (map); a side
arm reads 4 K (+ 4 written by the map) and (M + Nt) Q floats per row slice, which vanish per trial.

The run FAILS (non-zero exit, after the document is written) if a side record, fit or mapped matrix is not bit-identical to
its matrix arm's.

usage: fusion_side_bench.py [M Nt] [--reps 7] [--operands M Nt] [--out FILE.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _clock():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln.lower()][:2]
    except Exception as ex:      # noqa: BLE001 -- the clock line is a note, not a measurement
        return ["not read: %s" % ex]


def _one(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "spread_max_over_min": float(max(ms) / min(ms)),
            "reps": len(ms)}


def alternate(side, matrix, reps, warmup=2):
    """warm both, then side, matrix, side, matrix ..."""
    import torch
    for _ in range(warmup):
        side()
        matrix()
    torch.cuda.synchronize()
    ts, tm = [], []
    for _ in range(reps):
        ts.append(_one(side))
        tm.append(_one(matrix))
    out = {"side": _stats(ts), "matrix": _stats(tm)}
    out["side_over_matrix"] = out["side"]["median_ms"] / out["matrix"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("M", type=int, nargs="?", default=20000)
    ap.add_argument("Nt", type=int, nargs="?", default=20000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--operands", type=int, nargs=2, metavar=("M", "Nt"), help="time the operand-form fit at this size instead")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("fusion_side_bench.py: no GPU -- these are measurements, there is nothing to fall back to")
    from plda_amd import MPlda, fusion as FU
    dev = torch.device("cuda", 0)
    eng = MPlda(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    ops = ["min", "absdiff", "prod", "max", "sum", "min", "absdiff"]
    failures = []

    def qualities(m, nt, q):
        """q sides over log-durations; the seven pairs of vectors differ, so that no two sides are dependent"""
        out = []
        for j in range(q):
            e = torch.log(2.0 + 38.0 * torch.rand(m, dtype=torch.float32, device=dev, generator=g))
            t = torch.log(2.0 + 38.0 * torch.rand(nt, dtype=torch.float32, device=dev, generator=g))
            out.append(FU.Side(ops[j], e, t))
        return out

    def materialised(s):
        e, t = s.enrol[:, None], s.test[None, :]
        return {"min": lambda: torch.where(e < t, e, t), "max": lambda: torch.where(e > t, e, t), "sum": lambda: e + t,
                "absdiff": lambda: (e - t).abs(), "prod": lambda: e * t}[s.op]().expand(e.shape[0], t.shape[1]).contiguous()

    if args.operands:
        M, Nt = args.operands
        d, Q = 128, 3
        rng = np.random.default_rng(d)
        qm, _ = np.linalg.qr(rng.standard_normal((d, d)))
        eng.set_model(rng.random(d), qm * (1.0 + rng.random(d))[:, None], np.sort(0.05 + rng.random(d) * 4.0)[::-1].copy())
        spk_e, spk_t = torch.arange(M, device=dev) // 20, torch.arange(Nt, device=dev) // 20
        centres = torch.randn((max(M, Nt) // 20 + 1, d), dtype=torch.float64, device=dev, generator=g)
        U = centres[spk_e] + 0.7 * torch.randn((M, d), dtype=torch.float64, device=dev, generator=g)
        V = centres[spk_t] + 0.7 * torch.randn((Nt, d), dtype=torch.float64, device=dev, generator=g)
        sides = qualities(M, Nt, Q)
        last = {}

        def ofit():
            last["fit"] = FU.fit_from_operands_with_sides_dev(eng, U.data_ptr(), None, 1, M, V.data_ptr(), Nt, None, None, spk_e.data_ptr(),
                                                              spk_t.data_ptr(), sides)
        ofit()
        torch.cuda.synchronize()
        ms = [_one(ofit) for _ in range(max(2, args.reps // 3))]
        f = last["fit"]
        out = {"what": "plda_score_fusion_side_fit_dev", "M": M, "Nt": Nt, "d": d, "K": 1, "Q": Q, "ops": ops[:Q], "trials": M * Nt,
               "fit": _stats(ms), "ms_per_pass": float(np.median(ms)) / f.passes,
               "fit_result": {"a": f.a.tolist(), "b": f.b, "iterations": f.iterations, "passes": f.passes, "converged": f.converged,
                              "separable": f.separable, "cllr_after": f.cllr_after},
               "bytes_held": {"operands_and_sides": int(8 * d * (M + Nt) + 4 * Q * (M + Nt)), "matrix_form_would_hold": int(4 * M * Nt * (1 + Q))}}
    else:
        M, Nt = args.M, args.Nt
        es, ts = torch.arange(M, device=dev) // 20, torch.arange(Nt, device=dev) // 20
        S = torch.randn((M, Nt), dtype=torch.float32, device=dev, generator=g) * 2.0 - 1.0
        S += 2.5 * (es[:, None] == ts[None, :])
        sides7 = qualities(M, Nt, 7)
        mats = [materialised(s) for s in sides7]
        out_s, out_m = torch.empty_like(S), torch.empty_like(S)
        out = {"what": "the side kernels of csrc/fusion.hip against its matrix kernels on materialised sides", "M": M, "Nt": Nt, "trials": M * Nt, "ops": ops}
        c, theta = -0.4, 0.3
        for q in (3, 7):
            T = 1 + q
            a = np.array([0.15] + [0.05 * (-1.0) ** j for j in range(q)])
            sides = sides7[:q]
            ptrs, lds = [S.data_ptr()] + [x.data_ptr() for x in mats[:q]], [Nt] * T
            fus = FU.QualityFusion(a, c, ops[:q])
            last = {}

            def spass():
                last["s"] = FU.pass_with_sides_dev(eng, ptrs[:1], lds[:1], sides, M, Nt, es.data_ptr(), ts.data_ptr(), a, c, theta)

            def mpass():
                last["m"] = FU.pass_from_matrices_dev(eng, ptrs, lds, M, Nt, es.data_ptr(), ts.data_ptr(), a, c, theta)

            def smap():
                last["keep"] = FU.apply_with_sides_dev(eng, ptrs[:1], lds[:1], sides, M, Nt, fus, out_s.data_ptr(), Nt)

            def mmap():
                FU.apply_dev(eng, ptrs, lds, M, Nt, FU.Fusion(a, c), out_m.data_ptr(), Nt)

            key = "K1_Q%d_against_K%d" % (q, T)
            out["pass_" + key] = dict(alternate(spass, mpass, args.reps), bytes_per_trial={"side": 4, "matrix": 4 * T})
            if any(np.asarray(last["s"][k_]).tobytes() != np.asarray(last["m"][k_]).tobytes() for k_ in last["m"]):
                failures.append("pass %s: the side record is not the matrix record's bits" % key)
            out["map_" + key] = dict(alternate(smap, mmap, args.reps), bytes_per_trial={"side": 4 + 4, "matrix": 4 * T + 4})
            out["map_" + key]["bytes_ratio_matrix_over_side"] = (4 * T + 4) / 8.0
            out["map_" + key]["side_TBps"] = M * Nt * 8 / (out["map_" + key]["side"]["median_ms"] * 1e-3) / 1e12
            out["map_" + key]["matrix_TBps"] = M * Nt * (4 * T + 4) / (out["map_" + key]["matrix"]["median_ms"] * 1e-3) / 1e12
            torch.cuda.synchronize()
            if not torch.equal(out_s.view(torch.int32), out_m.view(torch.int32)):
                failures.append("map %s: the side map is not the matrix map's bits" % key)
            if q == 3:
                def sfit():
                    last["sf"] = FU.fit_with_sides_dev(eng, ptrs[:1], lds[:1], sides, M, Nt, es.data_ptr(), ts.data_ptr())

                def mfit():
                    last["mf"] = FU.fit_from_matrices_dev(eng, ptrs, lds, M, Nt, es.data_ptr(), ts.data_ptr())
                out["fit_" + key] = alternate(sfit, mfit, max(2, args.reps // 3), warmup=1)
                sf, mf = last["sf"], last["mf"]
                out["fit_" + key]["fit_result"] = {"a": sf.a.tolist(), "b": sf.b, "iterations": sf.iterations, "passes": sf.passes,
                                                  "converged": sf.converged, "cllr_after": sf.cllr_after}
                if sf.a.tobytes() != mf.a.tobytes() or sf.b != mf.b or sf.passes != mf.passes or sf.cllr_after != mf.cllr_after:
                    failures.append("fit %s: the side fit is not the matrix fit's bits" % key)
        out["bytes_held"] = {"one_system_and_7_sides": int(4 * M * Nt + 4 * 7 * (M + Nt)), "materialised": int(4 * M * Nt * 8)}
    out["shader_clock_after"] = _clock()
    out["failures"] = failures
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    if failures:
        sys.exit("fusion_side_bench.py: " + "; ".join(failures))


if __name__ == "__main__":
    main()
