"""PLDA domain adaptation measurements: whole calls between HIP events, warm-up, >= 5 timed
repetitions, medians; the shader clock the box reports right after the timed loops is recorded with them.

Statistics pass (plda_adapt_accumulate_dev on HBM-resident rows with weights) at 1e6 x 200, 1e6 x 512 and 2e5 x 1024.  Beside
the whole call, from the library's own trace spans of the SAME calls: the time inside syrk_f64 (the fit's weighted SYRK, code
this feature does not touch) and the time inside the centring kernel.  call / syrk is the price of reading the rows once
more to centre and augment them (plus the call's one synchronisation).

Update and blend (plda_adapt_update, plda_blend_model) at D = 200, 512, 1024 beside plda_fit_timings()[2] (GetOutput: one
simultaneous diagonalisation + the model export) of a fit at the same D in the same run; an update is an SPD inverse, one
more eigen-decomposition and ten D^3 products on top of that diagonalisation.

No threshold is fixed in advance: the document records, it does not judge.

usage: adapt_bench.py [--reps 5] [--out FILE.json]   (default: profiles/adapt_<host>.json)"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


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
    return _stats(ms)


def _clock():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln.lower()][:2]
    except Exception as ex:      # noqa: BLE001 -- the clock line is a note, not a measurement
        return ["not read: %s" % ex]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("adapt_bench.py: no GPU -- these are measurements, there is nothing to fall back to")
    import adapt_model as AM
    from plda_amd import MPlda
    dev = torch.device("cuda", 0)
    out = {"what": "plda_adapt_accumulate_dev / plda_adapt_update / plda_blend_model.  syrk_f64_ms_per_call is the trace span "
                   "of syrk_f64 INSIDE the same calls: it runs on the centred, augmented slab (width D + 1, once per slab), "
                   "not stand-alone on the raw rows, so call_over_syrk is the call against its own SYRK share, not against "
                   "a separate syrk_f64 of the rows (the library exports no entry point for that product alone)",
           "host": socket.gethostname(), "statistics": [], "update": []}
    for n, d in ((1000000, 200), (1000000, 512), (200000, 1024)):
        mean, T, psi = AM.synthetic_model(d, d)
        eng = MPlda(0)
        eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        eng.set_model(mean, T, psi)
        g = torch.Generator(device=dev)
        g.manual_seed(d)
        X = torch.randn((n, d), dtype=torch.float64, device=dev, generator=g) + torch.from_numpy(mean).to(dev) + 0.3
        w = torch.rand((n,), dtype=torch.float64, device=dev, generator=g)
        torch.cuda.synchronize()

        def acc():
            eng.adapt_reset()
            eng.adapt_accumulate_dev(X.data_ptr(), n, d, w.data_ptr())

        row = {"N": n, "D": d, "row_bytes": n * d * 8, "call": _timed(acc, args.reps)}
        eng.trace_enable(True)
        eng.trace_read(reset=True)
        for _ in range(args.reps):
            acc()
        spans = {s["name"].split(" ")[0]: s for s in eng.trace_read(reset=True)}
        eng.trace_enable(False)
        row["syrk_f64_ms_per_call"] = spans["adapt.syrk"]["ms"] / args.reps
        row["centre_ms_per_call"] = spans["adapt.centre"]["ms"] / args.reps
        row["slabs_per_call"] = spans["adapt.syrk"]["calls"] // args.reps
        row["call_over_syrk"] = row["call"]["median_ms"] / row["syrk_f64_ms_per_call"]
        row["call_TBps_of_rows_read_once"] = n * d * 8 / (row["call"]["median_ms"] * 1e-3) / 1e12
        out["statistics"].append(row)
        del X, w, eng
    for d in (200, 512, 1024):
        from conftest import make_data
        k = max(2 * d, 400)
        x, y = make_data(d, 5 * k, d, k, scale_between=0.5)
        eng = MPlda(0)
        fit_out = []
        for _ in range(args.reps + 1):
            eng.fit(x, y, 2)
            fit_out.append(eng.fit_timings()["output_ms"])
        m = eng.get_model()
        model = (m["mean"], m["transform"], m["psi"])
        z = 0.4 + 3.0 * np.random.default_rng(d).random((4 * d, d))
        eng.adapt_accumulate(z)
        st = eng.adapt_stats()

        def upd():
            eng.set_model(*model)
            eng.adapt_reset()
            eng.adapt_add_stats(st["tot_weight"], st["rows"], st["pilot"], st["s1"], st["s2"])
            t0 = time.perf_counter()
            eng.adapt_update()
            upd.ms.append((time.perf_counter() - t0) * 1e3)

        def bld():
            eng.set_model(*model)
            t0 = time.perf_counter()
            eng.blend(other, 0.5)
            bld.ms.append((time.perf_counter() - t0) * 1e3)

        other = AM.synthetic_model(d, 7)
        upd.ms, bld.ms = [], []
        for _ in range(args.reps + 1):
            upd()
            bld()
        out["update"].append({"D": d, "fit_getoutput": _stats(fit_out[1:]), "adapt_update": _stats(upd.ms[1:]),
                              "blend_model": _stats(bld.ms[1:]),
                              "update_over_getoutput": float(np.median(upd.ms[1:]) / np.median(fit_out[1:])),
                              "blend_over_getoutput": float(np.median(bld.ms[1:]) / np.median(fit_out[1:]))})
        del eng
    out["shader_clock_after"] = _clock()
    text = json.dumps(out, indent=1)
    print(text)
    path = args.out or os.path.join(ROOT, "profiles", "adapt_%s.json" % out["host"])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
