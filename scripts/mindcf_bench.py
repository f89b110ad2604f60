"""minDCF measurements: whole calls on the host clock (every call returns host results, so it
ends synchronised), warm-up, >= 5 timed repetitions, medians.

  matrix  on an M x Nt labelled Gaussian matrix (N(0, 1), targets shifted by 2.5, 20 utterances per speaker on both sides):
            plda_min_dcf_matrix_dev at the two NIST points and at five points, ALTERNATING with plda_eer_matrix_dev
            under PLDA_EER_VARIANT=1 (the three-pass EER: the same three reads by the EER's own kernel) in the same job;
            with --operands D the operand form on operands of that dimension (its own matrix); with --sort the only
            stock formulation that is exact, torch.sort of the keys + cumulative sums (20 000 x 20 000 fits; 1e10 does not).
  list    the list form on N scores (1 % targets), host arrays in, upload included.

usage: mindcf_bench.py matrix M Nt [--operands D] [--sort] [--reps 5] [--out FILE.json]
       mindcf_bench.py list N [--reps 5] [--out FILE.json]
One JSON document on stdout (and in --out).  The shader clock the box reports right after the timed loops is recorded with it."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NIST = ((0.01, 1.0, 1.0), (0.005, 1.0, 1.0))
FIVE = ((0.01, 1.0, 1.0), (0.05, 1.0, 1.0), (0.001, 1.0, 1.0), (0.5, 1.0, 1.0), (0.005, 10.0, 1.0))


def _engine(env=None, D=0):
    from plda_amd import MPlda
    for k, v in (env or {}).items():
        os.environ[k] = v
    eng = MPlda(0)
    for k in (env or {}):
        del os.environ[k]
    if D:
        rng = np.random.default_rng(D)
        q, _ = np.linalg.qr(rng.standard_normal((D, D)))
        eng.set_model(rng.random(D), q * (1.0 + rng.random(D))[:, None], np.sort(rng.random(D) * 4.0 + 0.05)[::-1].copy())
    return eng


def _stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def _alternate(fns, reps, warmup=1, device_sync=True):
    """{name: fn} timed in turn, reps rounds (device_sync: torch's own work has ended before the clock starts)."""
    if device_sync:
        import torch
    ms = {k: [] for k in fns}
    for r in range(warmup + reps):
        for k, fn in fns.items():
            if device_sync:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if r >= warmup:
                ms[k].append((t1 - t0) * 1e3)
    return {k: _stats(v) for k, v in ms.items()}


def _clock():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln.lower()][:2]
    except Exception as ex:      # noqa: BLE001 -- the clock line is a note, not a measurement
        return ["not read: %s" % ex]


def bench_matrix(a):
    import torch
    from plda_amd import dcf, eer
    dev = torch.device("cuda", 0)
    m, nt = a.M, a.Nt
    g = torch.Generator(device=dev); g.manual_seed(3)
    es = torch.randint(0, max(m // 20, 2), (m,), device=dev, generator=g)
    ts = torch.randint(0, max(m // 20, 2), (nt,), device=dev, generator=g)
    S = torch.empty((m, nt), dtype=torch.float32, device=dev)
    for r0 in range(0, m, 8192):                                   # (slab by slab: no second copy of 40 GB)
        r1 = min(m, r0 + 8192)
        S[r0:r1] = torch.randn((r1 - r0, nt), dtype=torch.float32, device=dev, generator=g)
        S[r0:r1] += 2.5 * (es[r0:r1, None] == ts[None, :]).float()
    torch.cuda.synchronize()
    eng, eng3 = _engine(), _engine({"PLDA_EER_VARIANT": "1"})
    args = (S.data_ptr(), nt, m, nt, es.data_ptr(), ts.data_ptr())
    doc = {"what": "matrix", "M": m, "Nt": nt, "trials": m * nt}
    res2, info2 = dcf.min_dcf_from_matrix_dev(eng, *args, points=NIST)
    res5, info5 = dcf.min_dcf_from_matrix_dev(eng, *args, points=FIVE)
    doc["nist"] = {"results": res2, "info": info2}
    doc["five"] = {"results": res5, "info": info5}
    doc["timing"] = _alternate({"min_dcf_2_points": lambda: dcf.min_dcf_from_matrix_dev(eng, *args, points=NIST),
                                "eer_three_passes": lambda: eer.eer_from_matrix_dev(eng3, *args),
                                "min_dcf_5_points": lambda: dcf.min_dcf_from_matrix_dev(eng, *args, points=FIVE)}, a.reps)
    doc["ratio_to_three_pass_eer"] = doc["timing"]["min_dcf_2_points"]["median_ms"] / doc["timing"]["eer_three_passes"]["median_ms"]
    if a.sort:
        def by_sort():
            tgt = (es[:, None] == ts[None, :]).reshape(-1)
            u = S.reshape(-1).view(torch.int32).to(torch.int64) & 0xffffffff
            key = torch.where(u >= 0x80000000, 0xffffffff - u, u + 0x80000000)
            key, order = torch.sort(key)
            cum_t = torch.cumsum(tgt[order].to(torch.int64), 0)
            n_pos = int(cum_t[-1]); n_neg = key.numel() - n_pos
            cum_n = torch.arange(1, key.numel() + 1, device=dev) - cum_t
            out = []
            for pi, cm, cf in NIST:                                # (every position as a cut: ties are not merged here)
                v = ((cm * pi) * cum_t.double()) / n_pos + ((cf * (1.0 - pi)) * (n_neg - cum_n).double()) / n_neg
                out.append(float(v.min()))
            return out
        doc["torch_sort"] = _alternate({"torch_sort_cumsum_2_points": by_sort}, max(2, a.reps // 2))["torch_sort_cumsum_2_points"]
        doc["ratio_torch_sort_to_min_dcf"] = doc["torch_sort"]["median_ms"] / doc["timing"]["min_dcf_2_points"]["median_ms"]
    if a.operands:
        D = a.operands
        engo = _engine(D=D)
        rng = np.random.default_rng(1)
        spk = torch.from_numpy(rng.standard_normal((max(m // 20, 2), D)) * 1.5).to(dev)
        U = spk[es] + torch.randn((m, D), dtype=torch.float64, device=dev, generator=g)
        V = spk[ts] + torch.randn((nt, D), dtype=torch.float64, device=dev, generator=g)
        torch.cuda.synchronize()
        oargs = (U.data_ptr(), None, 1, m, V.data_ptr(), nt, es.data_ptr(), ts.data_ptr())
        ores, oinfo = dcf.min_dcf_from_operands_dev(engo, *oargs, points=NIST)
        doc["operands"] = {"D": D, "results": ores, "info": oinfo,
                           "timing": _alternate({"min_dcf_operands_2_points": lambda: dcf.min_dcf_from_operands_dev(engo, *oargs, points=NIST)},
                                                a.reps)["min_dcf_operands_2_points"]}
    doc["clock"] = _clock()
    return doc


def bench_list(a):
    from plda_amd import dcf
    rng = np.random.default_rng(5)
    n_pos = max(a.N // 100, 1)
    pos = rng.normal(2.5, 1.0, n_pos).astype(np.float32)
    neg = rng.normal(0.0, 1.0, a.N - n_pos).astype(np.float32)
    eng = _engine()
    res, info = dcf.min_dcf_from_lists(eng, pos, neg, NIST)
    doc = {"what": "list", "N": a.N, "results": res, "info": info,
           "timing": _alternate({"min_dcf_lists_2_points": lambda: dcf.min_dcf_from_lists(eng, pos, neg, NIST)}, a.reps,
                                device_sync=False)["min_dcf_lists_2_points"]}
    doc["clock"] = _clock()
    return doc


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    pm = sub.add_parser("matrix")
    pm.add_argument("M", type=int); pm.add_argument("Nt", type=int)
    pm.add_argument("--operands", type=int, default=0); pm.add_argument("--sort", action="store_true")
    pl = sub.add_parser("list")
    pl.add_argument("N", type=int)
    for p in (pm, pl):
        p.add_argument("--reps", type=int, default=5); p.add_argument("--out", default=None)
    a = ap.parse_args()
    doc = bench_matrix(a) if a.cmd == "matrix" else bench_list(a)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
