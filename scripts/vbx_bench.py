"""VBx resegmentation measurements: whole plda_vbx_dev calls between HIP events, warm-up, timed
repetitions, medians; the shader clock the box reports right after the timed loops is recorded with them.

Seeded recordings from the generator of tests/vbx_model.py: D = 128, 5 planted speakers, S = 10 over-split initial speakers,
10 fixed iterations (epsilon = -inf).  Shapes: R = 2 000 recordings of T = 100 segments (LDS class), R = 200 of T = 1 000 and
R = 16 of T = 4 096 (HBM class).  Recorded per shape:
  device      plda_vbx_dev on vectors, labels and outputs in HBM (check kernel, the call's two waits, the iterations)
  chain_step  an UPPER bound on the cycles one chain step costs, derived from the whole call: time x clock / (iterations x T x
              rounds), rounds = ceil(R / compute units) -- everything else of an iteration is inside it
  torch       the same iteration in stock torch fp64 operations on the same GPU, batched over the recordings, a Python loop
              over the T dependent steps of the forward and the backward pass
  model       tests/vbx_model.py (NumPy, fp64) on the host, one thread, on at most --model-recs recordings, scaled to R
The two are what a user has today; labels are compared with the device's and counted, not asserted.
No ratio is fixed in advance: the document records, it does not judge.

usage: vbx_bench.py [--reps 5] [--shapes 2000x100,200x1000,16x4096] [--no-torch] [--no-model] [--model-recs 8] [--out FILE.json]
       (default: profiles/vbx_<R>x<T>.json per shape)"""
import argparse
import json
import os
import re
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

D, K, S, ITERS = 128, 5, 10, 10
FA, FB, P, SIGMA = 0.3, 17.0, 0.99, 5.0


def _stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def _timed(fn, reps, warmup=1):
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


def _mhz(lines):
    for ln in lines:
        m = re.search(r"\((\d+)\s*Mhz\)", ln, re.I)
        if m:
            return float(m.group(1))
    return None


def torch_vbx(y, labels, phi, iters):
    """the contract in stock torch fp64 operations, batched over R recordings of one T: y [R, T, D], labels [R, T] -> labels"""
    import torch
    r, t, d = y.shape
    s = int(labels.max()) + 1
    rho = y * phi.sqrt()
    g = -0.5 * ((y * y).sum(-1) + d * np.log(2 * np.pi))
    es = float(np.exp(SIGMA))
    gamma = torch.full((r, t, s), 1.0 / (es + s - 1), dtype=torch.float64, device=y.device)
    gamma.scatter_(2, labels.long().unsqueeze(-1), es / (es + s - 1))
    pi = torch.full((r, s), 1.0 / s, dtype=torch.float64, device=y.device)
    fafb = FA / FB
    for _ in range(iters):
        n = gamma.sum(1)
        inv_l = 1.0 / (1.0 + fafb * n.unsqueeze(-1) * phi)
        alpha = fafb * inv_l * (gamma.transpose(1, 2) @ rho)
        lp = FA * (rho @ alpha.transpose(1, 2) - 0.5 * ((inv_l + alpha * alpha) @ phi).unsqueeze(1) + g.unsqueeze(-1))
        m = lp.max(-1, keepdim=True).values
        b = (lp - m).exp()
        a, beta, c = torch.empty_like(b), torch.ones_like(b), torch.empty_like(g)
        u = b[:, 0] * pi
        c[:, 0] = u.sum(-1)
        a[:, 0] = u / c[:, :1]
        q1 = (1 - P) * pi
        for j in range(1, t):
            u = b[:, j] * (P * a[:, j - 1] + q1)
            cj = u.sum(-1, keepdim=True)
            c[:, j] = cj[:, 0]
            a[:, j] = u / cj
        for j in range(t - 2, -1, -1):
            w = b[:, j + 1] * beta[:, j + 1]
            beta[:, j] = (P * w + (1 - P) * (pi * w).sum(-1, keepdim=True)) / c[:, j + 1:j + 2]
        gamma = a * beta
        pin = gamma[:, 0] + (1 - P) * pi * (b[:, 1:] * beta[:, 1:] / c[:, 1:].unsqueeze(-1)).sum(1)
        pi = pin / pin.sum(-1, keepdim=True)
    return gamma.argmax(-1)


def measure(r, t, reps, with_torch, with_model, model_recs):
    import torch
    import vbx_model as M
    from plda_amd import MPlda, diarize
    dev = torch.device("cuda", 0)
    eng = MPlda(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    eng.set_model(np.zeros(4), np.eye(4), np.ones(4))
    ys, ls = [], []
    for q in range(r):
        y, lab, _, phi = M.generate(t, D, K, S, 10_000 * t + q)
        ys.append(y)
        ls.append(lab)
    y, lab = np.concatenate(ys), np.concatenate(ls)
    offsets = diarize.offsets_of([t] * r)
    dY, dL, dPhi = torch.from_numpy(y).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(phi).to(dev)
    oL = torch.empty(r * t, dtype=torch.int32, device=dev)
    oK = torch.empty(r, dtype=torch.int32, device=dev)

    def device():
        eng.vbx_dev(dY.data_ptr(), D, dPhi.data_ptr(), dL.data_ptr(), offsets, oL.data_ptr(), oK.data_ptr(), FA, FB, P, SIGMA, ITERS,
                    float("-inf"))

    res = {"what": "VBx resegmentation, %d fixed iterations" % ITERS, "host": socket.gethostname(), "R": r, "T": t, "D": D, "S": S,
           "planted_speakers": K, "params": [FA, FB, P, SIGMA], "class": diarize.vbx_plan(eng, t, S, D)}
    res["device"] = _timed(device, reps)
    torch.cuda.synchronize()
    labels_d = oL.cpu().numpy().copy()
    res["clock_after"] = _clock()
    mhz = _mhz(res["clock_after"])
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    rounds = -(-r // cus)
    res["chain_step"] = {"compute_units": cus, "rounds": rounds, "clock_mhz": mhz,
                         "cycles_upper_bound": None if mhz is None else res["device"]["median_ms"] * 1e-3 * mhz * 1e6 / (ITERS * t * rounds)}
    res["clusters_per_recording"] = {"min": int(oK.min()), "max": int(oK.max())}
    if with_torch:
        ty, tl = dY.view(r, t, D), dL.view(r, t)
        out = {}

        def stock():
            out["labels"] = torch_vbx(ty, tl, dPhi, ITERS)

        res["torch"] = _timed(stock, max(1, min(reps, 2)), warmup=1)
        raw = out["labels"].cpu().numpy()
        same = sum(np.array_equal(M.first_member_labels(raw[q])[0], labels_d[q * t:(q + 1) * t]) for q in range(r))
        res["torch"]["recordings_with_the_device_labels"] = int(same)
        res["torch_over_device"] = res["torch"]["median_ms"] / res["device"]["median_ms"]
    if with_model:
        n = min(r, model_recs)
        t0 = time.perf_counter()
        same = 0
        for q in range(n):
            w = M.run(ys[q], ls[q], phi, FA, FB, P, SIGMA, ITERS, -np.inf)
            same += np.array_equal(w["labels"], labels_d[q * t:(q + 1) * t])
        ms = 1e3 * (time.perf_counter() - t0)
        res["model"] = {"recordings_run": n, "ms": ms, "scaled_to_R_ms": ms * r / n, "threads": 1,
                        "recordings_with_the_device_labels": int(same)}
        res["model_over_device"] = res["model"]["scaled_to_R_ms"] / res["device"]["median_ms"]
    del eng
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="2000x100,200x1000,16x4096")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--model-recs", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("vbx_bench.py: no GPU -- these are measurements, there is nothing to fall back to")
    for shape in args.shapes.split(","):
        r, t = (int(v) for v in shape.split("x"))
        res = measure(r, t, args.reps, not args.no_torch, not args.no_model, args.model_recs)
        path = args.out or os.path.join(ROOT, "profiles", "vbx_%dx%d.json" % (r, t))
        if args.out and len(args.shapes.split(",")) > 1:
            path = "%s.%dx%d.json" % (os.path.splitext(args.out)[0], r, t)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({k: res[k] for k in res if k not in ("what", "host")}), flush=True)


if __name__ == "__main__":
    main()
