"""Embedding-chain measurements: whole plda_embed_apply_dev calls between HIP events, warm-up, timed
repetitions, medians; the shader clock the box reports right after the timed loops is recorded with them.

Shapes (rows x Din -> Dout, input dtype): 100 000 x 512 -> 200 fp32, 1 200 000 x 256 -> 128 fp32, 100 000 x 200 -> 200 fp64 (class 1,
the Kaldi recipe: m_in, A, sqrt(Dout)), 1 000 000 x 512 without A (class 0: m_in, sqrt(D)).  Recorded per shape:
  device      plda_embed_apply_dev as dispatched (plda_embed_plan's class)
  forced      the same chain on a handle created with PLDA_EMBED_VARIANT=1: row pass + fp64 GEMM + row pass (class 2); shapes with A
  torch       the same chain in stock torch fp64 operations on the same GPU
  class 1     fraction of the fp64 MFMA peak (2 R Din Dout flop over 78.6 TFLOP/s, the figure bench.py uses), beside
              transform_fused_kernel's own fraction at the nearest D from the README
  class 0     fraction of the HBM bandwidth (bytes read + written over 8 TB/s)
plus embed_fit at 100 000 x 512 -> 200, 5 000 speakers, kinds 1 and 2, timed once each (--no-fit skips), and the worst ratio to
the a-priori bound per class over a few small chains (profiles/embed_parity.json; tests/embed_model.py).
No speed is fixed in advance; the one condition is relative: class 1 against the forced class-2 arm, same box, same session.

usage: embed_bench.py [--reps 5] [--shapes all] [--no-torch] [--no-fit] [--no-parity]   (profiles/embed_<shape>.json per shape)"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(100_000, 512, 200, "f32", True), (1_200_000, 256, 128, "f32", True), (100_000, 200, 200, "f64", True),
          (1_000_000, 512, 512, "f32", False)]
K4_FRACTION = {200: 0.54, 128: 0.76, 256: 0.76, 512: 0.78}     # README: transform_fused_kernel at 100k x 200 / 1.2M x 256 / 1M x 512
HBM_BYTES_PER_S = 8.0e12
PEAK_FP64_MFMA_FLOPS = 78.6e12                                  # v_mfma_f64_16x16x4_f64 (bench.py)


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


def _engine(forced):
    import torch
    from plda_amd import MPlda
    if forced:
        os.environ["PLDA_EMBED_VARIANT"] = "1"
    try:
        eng = MPlda(0)
    finally:
        os.environ.pop("PLDA_EMBED_VARIANT", None)
    eng.set_stream(torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream)
    return eng


def _plan(eng, din, dout, has_a, dtype):
    import ctypes as C
    out = np.zeros(3, np.int32)
    eng._ck(eng._lib.plda_embed_plan(eng._h, din, dout, int(has_a), dtype, out.ctypes.data_as(C.c_void_p)))
    return {"class": int(out[0]), "rows_per_workgroup": int(out[1]), "lds_bytes": int(out[2])}


def measure(r, din, dout, dt, has_a, reps, with_torch):
    import torch
    from plda_amd.embed import EmbeddingChain
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(r + din)
    m_in = rng.standard_normal(din)
    A = rng.standard_normal((dout, din)) / np.sqrt(din) if has_a else None
    chain = EmbeddingChain(m_in, 0.0, A, None, float(np.sqrt(dout)))
    tdt = torch.float32 if dt == "f32" else torch.float64
    g = torch.Generator(device=dev)
    g.manual_seed(r)
    dX = torch.randn((r, din), dtype=tdt, device=dev, generator=g)
    dO = torch.empty((r, dout), dtype=torch.float64, device=dev)
    code = 1 if dt == "f32" else 0
    res = {"what": "embedding chain (m_in, %s, sqrt(Dout))" % ("A" if has_a else "no A"), "R": r, "Din": din, "Dout": dout, "dtype": dt}
    outs = {}
    for name in ("device", "forced") if has_a else ("device",):
        eng = _engine(name == "forced")
        eng.set_embedding(chain)
        res[name + "_plan"] = _plan(eng, din, dout, has_a, code)
        res[name] = _timed(lambda: eng.embed_dev(dX.data_ptr(), code, r, din, dO.data_ptr()), reps)
        torch.cuda.synchronize()
        outs[name] = dO[:4096].cpu().numpy().copy()
        del eng
    res["clock_after"] = _clock()
    res["clock_mhz"] = _mhz(res["clock_after"])
    ms = res["device"]["median_ms"]
    if has_a:
        res["forced_over_device"] = res["forced"]["median_ms"] / ms
        res["max_abs_difference_of_the_two_arms"] = float(np.max(np.abs(outs["device"] - outs["forced"])))
        flop = 2.0 * r * din * dout
        res["fp64_mfma_peak_fraction"] = flop / (ms * 1e-3) / PEAK_FP64_MFMA_FLOPS
        res["forced_fp64_mfma_peak_fraction"] = flop / (res["forced"]["median_ms"] * 1e-3) / PEAK_FP64_MFMA_FLOPS
        res["transform_fused_kernel_fraction_at_nearest_D"] = K4_FRACTION.get(dout)
    else:
        moved = r * din * ((4 if dt == "f32" else 8) + 8.0)
        res["hbm_fraction"] = moved / (ms * 1e-3) / HBM_BYTES_PER_S
    if with_torch:
        tm, tA = torch.from_numpy(m_in).to(dev), (torch.from_numpy(A).to(dev) if has_a else None)
        keep = {}

        def stock():
            v = dX.double() - tm
            u = v @ tA.T if tA is not None else v
            keep["out"] = u * (float(np.sqrt(dout)) / u.norm(dim=1, keepdim=True))

        res["torch"] = _timed(stock, reps)
        res["torch_over_device"] = res["torch"]["median_ms"] / ms
        res["max_abs_difference_to_torch"] = float(np.max(np.abs(keep["out"][:4096].cpu().numpy() - outs["device"])))
    return res


def measure_fit():
    import torch
    eng = _engine(False)
    rng = np.random.default_rng(7)
    n, d, dout, k = 100_000, 512, 200, 5_000
    lab = (np.arange(n) % k).astype(np.uint64)
    x = (rng.standard_normal((k, d))[lab.astype(np.int64)] * 2.0 + rng.standard_normal((n, d))).astype(np.float32)
    res = {"what": "plda_embed_fit (host arrays: upload included), timed once each", "N": n, "Din": d, "Dout": dout, "speakers": k}
    for kind in ("whiten", "lda"):
        t0 = time.perf_counter()
        eng.fit_embedding(x, lab.astype(np.uint32), kind, dout, 0.0, None)
        torch.cuda.synchronize()
        res[kind + "_ms"] = 1e3 * (time.perf_counter() - t0)
    res["clock_after"] = _clock()
    return res


def measure_parity():
    """worst ratio of |device - longdouble model| to the a-priori bound, per class, over the six chain forms at a few shapes"""
    import embed_model as em
    from test_embed_model import FORMS, make_chain
    from plda_amd.embed import EmbeddingChain
    worst = {}
    for forced in (False, True):
        eng = _engine(forced)
        for din, dout in ((7, 15), (200, 150), (256, 200), (520, 512), (520, 513)):
            rng = np.random.default_rng(din + dout)
            for form in FORMS:
                for offset in (0.0, 1e5):
                    ch = make_chain(form, din, dout, rng, offset)
                    eng.set_embedding(EmbeddingChain(ch.m_in, ch.len_in, ch.A, ch.m_out, ch.len_out, dim=din))
                    cls = _plan(eng, din, dout if ch.A is not None else din, ch.A is not None, 0)["class"]
                    for dt in (np.float32, np.float64):
                        x = (rng.standard_normal((40, din)) + offset).astype(dt)
                        err = np.abs(np.asarray(eng.embed(x), np.longdouble) - em.apply(ch, x, np.longdouble)).astype(np.float64)
                        key = "class %d%s" % (cls, " (forced)" if forced and ch.A is not None else "")
                        worst[key] = max(worst.get(key, 0.0), float(np.max(err / em.error_bound(ch, x))))
        del eng
    return {"what": "worst |device - model| / bound per dispatch class (tests/embed_model.py: error_bound)", "worst_ratio": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="all", help="all, none, or indices into the shape list, e.g. 0,2")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--no-parity", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("embed_bench.py: no GPU -- these are measurements, there is nothing to fall back to")
    prof = os.path.join(ROOT, "profiles")
    os.makedirs(prof, exist_ok=True)

    def write(name, res):
        with open(os.path.join(prof, name), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({k: v for k, v in res.items() if k != "what"}), flush=True)

    sel = [] if args.shapes == "none" else range(len(SHAPES)) if args.shapes == "all" else [int(v) for v in args.shapes.split(",")]
    for i in sel:
        r, din, dout, dt, has_a = SHAPES[i]
        write("embed_%dx%d_%s_%s.json" % (r, din, str(dout) if has_a else "noA", dt), measure(r, din, dout, dt, has_a, args.reps, not args.no_torch))
    if not args.no_fit:
        write("embed_fit_100000x512_200.json", measure_fit())
    if not args.no_parity:
        write("embed_parity.json", measure_parity())


if __name__ == "__main__":
    main()
