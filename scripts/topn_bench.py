"""Top-N retrieval measurements: whole calls between HIP events, warm-up, >= 5 timed repetitions, medians.

plda_score_topn_dev on M x Nt (D), per axis (0: per row, 1: per column) and n, against two things measured in the same job:
  (a) the floor: plda_score_matrix_dev alone into one reused slab, over the same slabs (the scores must be produced)
      -> added time = t_topn - t_gemm, and the bytes per second it stands for at the 8 B per score a two-read selection needs;
  (b) what a caller could do before: the same slabs through torch.topk -- along the row for axis 0; for axis 1 along the column
      of every slab, merged into the running result with torch.cat + topk.
The torch path breaks ties as it likes, so its result is compared by VALUE only (max |score difference|).

usage: topn_bench.py M Nt D [--n 10,100] [--axes 0,1] [--reps 5] [--out FILE.json]
One JSON document on stdout (and in --out).  The shader clock the box reports right after the timed loops is recorded with it."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from asnorm_bench import _clock, _default_slab_rows, _engine, _timed      # noqa: E402 -- the same harness as the AS-norm figures


def run(args):
    import torch
    dev = torch.device("cuda", 0)
    M, Nt, D = args.M, args.Nt, args.D
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    U = torch.randn((M, D), dtype=torch.float64, device=dev, generator=g)
    V = torch.randn((Nt, D), dtype=torch.float64, device=dev, generator=g)
    eng = _engine(D)
    rows = _default_slab_rows(M, Nt)
    slab = torch.empty((rows, Nt), dtype=torch.float32, device=dev)
    out = {"what": "plda_score_topn_dev", "M": M, "Nt": Nt, "D": D, "slab_rows": rows, "scores": M * Nt, "score_bytes": M * Nt * 4}

    def gemm_only():
        for r0 in range(0, M, rows):
            m = min(rows, M - r0)
            eng.score_matrix_dev(U[r0:r0 + m].data_ptr(), None, 1, m, V.data_ptr(), Nt, slab.data_ptr(), Nt)

    out["gemm_only_same_slabs"] = _timed(gemm_only, args.reps)
    tg = out["gemm_only_same_slabs"]["median_ms"]
    for axis in [int(a) for a in args.axes.split(",")]:
        lines = M if axis == 0 else Nt
        for n in [int(x) for x in args.n.split(",")]:
            os_ = torch.empty((lines, n), dtype=torch.float32, device=dev)
            oi = torch.empty((lines, n), dtype=torch.int64, device=dev)
            base = {}

            def call():
                eng.score_topn_dev(U.data_ptr(), None, 1, M, V.data_ptr(), Nt, axis, n, os_.data_ptr(), oi.data_ptr())

            def gemm_topk():
                run_v = run_i = None
                for r0 in range(0, M, rows):
                    m = min(rows, M - r0)
                    eng.score_matrix_dev(U[r0:r0 + m].data_ptr(), None, 1, m, V.data_ptr(), Nt, slab.data_ptr(), Nt)
                    if axis == 0:
                        v, i = torch.topk(slab[:m], n, dim=1)
                        run_v = v if run_v is None else torch.cat([run_v, v], dim=0)
                        run_i = i if run_i is None else torch.cat([run_i, i], dim=0)
                    else:
                        v, i = torch.topk(slab[:m], min(n, m), dim=0)
                        i = i + r0
                        if run_v is not None:
                            v, i = torch.cat([run_v, v], dim=0), torch.cat([run_i, i], dim=0)
                            v, sel = torch.topk(v, n, dim=0)
                            i = torch.gather(i, 0, sel)
                        run_v, run_i = v, i
                base["v"] = run_v if axis == 0 else run_v.t()

            rec = {"topn": _timed(call, args.reps), "gemm_plus_torch_topk_same_slabs": _timed(gemm_topk, args.reps),
                   "topn_again": _timed(call, args.reps)}     # alternated: the spread between two windows of one code
            t, tb = rec["topn"]["median_ms"], rec["gemm_plus_torch_topk_same_slabs"]["median_ms"]
            rec["added_ms_over_gemm"] = t - tg
            rec["added_over_gemm"] = t / tg - 1.0
            rec["speedup_over_torch_topk"] = tb / t
            rec["select_GBps_at_8_bytes_per_score"] = M * Nt * 8 / ((t - tg) * 1e-3) / 1e9 if t > tg else None
            call()
            torch.cuda.synchronize()
            rec["max_abs_score_difference_to_torch_topk"] = float((os_ - base["v"]).abs().max())
            out["axis%d_n%d" % (axis, n)] = rec
    out["gemm_only_same_slabs_again"] = _timed(gemm_only, args.reps)
    out["shader_clock_after"] = _clock()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("M", type=int)
    ap.add_argument("Nt", type=int)
    ap.add_argument("D", type=int)
    ap.add_argument("--n", default="10,100")
    ap.add_argument("--axes", default="0,1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("topn_bench.py: no GPU -- these are measurements, there is nothing to fall back to")
    res = run(args)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
