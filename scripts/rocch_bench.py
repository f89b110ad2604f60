"""ROC-convex-hull measurements: whole calls on the host clock with both waits included (every
call returns host results, so it ends synchronised), warm-up, >= 5 timed repetitions, medians.

  matrix  on an M x Nt labelled Gaussian matrix (N(0, 1), targets shifted by --shift, default 2.5; 20 utterances per speaker
            on both sides: one trial in M / 20 is a target): plda_rocch_matrix_dev ALTERNATING with plda_eer_matrix_dev
            and plda_min_dcf_matrix_dev at the two NIST points on the same buffer in the same job (neither runs anything the
            hull touches, so this library's are the parent's); plda_pav_map_dev ALTERNATING with plda_affine_map_dev (out of
            place, the same two buffers); the per-pass times from the library's trace spans of one more call; with --sort
            torch.sort of the keys + cumulative sums + the host hull (plda_rocch_hull) as the stock exact formulation
            (20 000 x 20 000 fits; 1e10 does not).  --shift 1 is the deliberately poor system (class means one standard
            deviation apart): the slow side.
  list    the list form on N scores (1 % targets), host arrays in, upload included.

usage: rocch_bench.py matrix M Nt [--shift 2.5] [--sort] [--reps 5] [--out FILE.json]
       rocch_bench.py list N [--reps 5] [--out FILE.json]
One JSON document on stdout (and in --out).  The shader clock the box reports right after the timed loops is recorded with it."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mindcf_bench import NIST, _alternate, _clock, _engine      # noqa: E402


def _shares(info, res):
    other = max(res["Np"], res["Nn"])
    return {"T": info["t_distinct"], "t_raw": info["t_raw"], "window_share": info["n_lds"] / other,
            "global_atomic_share": info["n_global_atomic"] / other, "register_share": info["n_register"] / other}


def bench_matrix(a):
    import torch
    from plda_amd import calibration as CB
    from plda_amd import dcf, eer
    from plda_amd import rocch as R
    dev = torch.device("cuda", 0)
    m, nt = a.M, a.Nt
    g = torch.Generator(device=dev); g.manual_seed(3)
    es = torch.randint(0, max(m // 20, 2), (m,), device=dev, generator=g)
    ts = torch.randint(0, max(m // 20, 2), (nt,), device=dev, generator=g)
    S = torch.empty((m, nt), dtype=torch.float32, device=dev)
    for r0 in range(0, m, 8192):                                   # (slab by slab: no second copy of 40 GB)
        r1 = min(m, r0 + 8192)
        S[r0:r1] = torch.randn((r1 - r0, nt), dtype=torch.float32, device=dev, generator=g)
        S[r0:r1] += a.shift * (es[r0:r1, None] == ts[None, :]).float()
    torch.cuda.synchronize()
    eng = _engine()
    args = (S.data_ptr(), nt, m, nt, es.data_ptr(), ts.data_ptr())
    res, pav, info = R.rocch_from_matrix_dev(eng, *args)
    doc = {"what": "matrix", "M": m, "Nt": nt, "trials": m * nt, "shift": a.shift, "result": res, "info": info, "shares": _shares(info, res)}
    doc["timing"] = _alternate({"rocch": lambda: R.rocch_from_matrix_dev(eng, *args),
                                "eer": lambda: eer.eer_from_matrix_dev(eng, *args),
                                "min_dcf_2_points": lambda: dcf.min_dcf_from_matrix_dev(eng, *args, points=NIST)}, a.reps)
    eng.trace_enable(True)
    R.rocch_from_matrix_dev(eng, *args)
    doc["passes"] = [s for s in eng.trace_read() if s["name"].startswith("rocch.")]
    eng.trace_enable(False)
    # the maps, out of place into a second matrix where one fits beside the first (1e10 trials: in place, twice each)
    cal = CB.Calibration(1.25, -0.5)
    out = torch.empty_like(S) if m * nt <= 1 << 32 else S
    ld_out = nt

    def pav_map():
        pav.apply_dev(eng, S.data_ptr(), nt, m, nt, out.data_ptr(), ld_out, bound=30.0)
        eng.synchronize()

    def affine_map():
        CB.apply_dev(eng, S.data_ptr(), nt, m, nt, cal, out.data_ptr(), ld_out)
        eng.synchronize()

    if out is not S:
        doc["map_timing"] = _alternate({"pav_map": pav_map, "affine_map": affine_map}, a.reps)
        doc["map_segments"] = int(len(pav.llr))
    if a.sort:
        def by_sort():
            tgt = (es[:, None] == ts[None, :]).reshape(-1)
            u = S.reshape(-1).view(torch.int32).to(torch.int64) & 0xffffffff
            key = torch.where(u >= 0x80000000, 0xffffffff - u, u + 0x80000000)
            key, order = torch.sort(key)
            cum_t = torch.cumsum(tgt[order].to(torch.int64), 0)
            last = torch.ones_like(key, dtype=torch.bool)
            last[:-1] = key[1:] != key[:-1]                         # one point per distinct key
            k = key[last].cpu().numpy().astype(np.uint32)
            y = cum_t[last].cpu().numpy().astype(np.uint64)
            x = (torch.nonzero(last).reshape(-1) + 1).cpu().numpy().astype(np.uint64) - y
            # every key as an "edge" key of the targets' side: the host hull on the full ROC
            ylt, xlt = np.concatenate([[0], y[:-1]]).astype(np.uint64), np.concatenate([[0], x[:-1]]).astype(np.uint64)
            keep = y > ylt                                          # the keys that hold a target
            return R.host_hull(k[keep], xlt[keep], x[keep], ylt[keep], y[keep], 1, int(y[-1]), int(x[-1]))[1]
        ref = by_sort()
        doc["torch_sort"] = dict(_alternate({"torch_sort_cumsum_host_hull": by_sort}, max(2, a.reps // 2))["torch_sort_cumsum_host_hull"],
                                 min_cllr=ref["min_cllr"], n_vertices=ref["n_vertices"], agrees=bool(ref["min_cllr"] == res["min_cllr"]))
    doc["clock"] = _clock()
    return doc


def bench_list(a):
    from plda_amd import rocch as R
    rng = np.random.default_rng(5)
    n_pos = max(a.N // 100, 1)
    pos = rng.normal(2.5, 1.0, n_pos).astype(np.float32)
    neg = rng.normal(0.0, 1.0, a.N - n_pos).astype(np.float32)
    eng = _engine()
    res, _, info = R.rocch_from_lists(eng, pos, neg)
    doc = {"what": "list", "N": a.N, "result": res, "info": info, "shares": _shares(info, res),
           "timing": _alternate({"rocch_lists": lambda: R.rocch_from_lists(eng, pos, neg)}, a.reps, device_sync=False)["rocch_lists"]}
    doc["clock"] = _clock()
    return doc


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    pm = sub.add_parser("matrix")
    pm.add_argument("M", type=int); pm.add_argument("Nt", type=int)
    pm.add_argument("--shift", type=float, default=2.5); pm.add_argument("--sort", action="store_true")
    pl = sub.add_parser("list")
    pl.add_argument("N", type=int)
    for p in (pm, pl):
        p.add_argument("--reps", type=int, default=5); p.add_argument("--out", default=None)
    a = ap.parse_args()
    doc = bench_matrix(a) if a.cmd == "matrix" else bench_list(a)
    doc["when"] = time.strftime("%Y-%m-%d %H:%M:%S %Z")
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
