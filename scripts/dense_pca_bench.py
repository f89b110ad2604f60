"""Dense scoring behind a per-recording PCA: whole calls from HBM-resident rows between HIP events, warm-up,
>= 5 timed repetitions, medians; the shader clock the box reports right after the timed loops is recorded with them.

Seeded recordings as in ahc_bench.py (2 .. 8 speakers of unequal segment counts, a speaker centre plus unit noise), D = 128.
Shapes: R = 2 000 recordings of N = 100 segments (LDS class, Gram route), R = 200 of N = 1 000 and R = 16 of N = 4 096 (HBM
class, covariance route), each at target energies 0.1 and 0.5.  Timed separately:
  score        plda_score_dense_pca_dev: every block written to HBM (count kernel + one kernel per class and scratch group)
  score_ahc    plda_score_dense_pca_ahc_dev at a score threshold of 0: the same blocks into the slab, clustered, dropped
  plain_ahc    plda_score_ahc_dev on the same buffer (NO PCA: one trials-GEMM call per recording, then the same clustering) --
               the path a caller had before; it reads the buffer as already-transformed vectors, which changes what the numbers
               mean but not what the call costs
  numpy        tests/dense_pca_model.py on the host, BLAS pinned to one thread (threadpoolctl), PCA and subspace model from the
               model's own functions, the N x N block in the GEMM form of the same LLR (the model's [N, N, d] broadcast does not
               fit in memory at N = 4 096); timed on the first `numpy_recordings` recordings and scaled to R, said so in the file
No ratio is fixed in advance: the document records, it does not judge.

It also writes profiles/dense_pca_parity.json: the ill-conditioned case of tests/test_gpu_dense_pca.py -- the spread between
the model's eigh and SVD routes, and the device's deviation from the eigh route (blocks after their fp32 rounding; eigenvalues
in fp64).

usage: dense_pca_bench.py [--reps 5] [--shapes 2000x100,200x1000,16x4096] [--targets 0.1,0.5] [--no-numpy] [--no-parity]"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from ahc_bench import D, _clock, _timed, recordings, synthetic_model   # noqa: E402


def numpy_call(model, x, offsets, target, count):
    """ms of the NumPy model on the first `count` recordings, one BLAS thread."""
    import dense_pca_model as dm
    from threadpoolctl import threadpool_limits
    with threadpool_limits(limits=1):
        t0 = time.perf_counter()
        wb = dm.model_covariances(model)
        t_model = time.perf_counter() - t0
        t0 = time.perf_counter()
        for r in range(count):
            xr = x[offsets[r]:offsets[r + 1]]
            lam, vecs = dm.pca(xr)
            d = dm.retained(lam, target)
            if d == 0:
                continue
            M, psi = dm.subspace_model(wb[0], wb[1], vecs[:d])
            y = (xr - model["mean"]) @ M.T
            y = y * np.sqrt(d / (y * y / (psi + 1.0)).sum(1))[:, None]
            c = psi / (psi + 1.0)
            var = 1.0 + c
            a1, a2 = c * y / var, -0.5 * (1.0 / var - 1.0 / (1.0 + psi))
            rr = -0.5 * (np.log(var).sum() - np.log(1.0 + psi).sum() + (c * c * y * y / var).sum(1))
            (a1 @ y.T + a2[None, :] @ (y * y).T + rr[:, None]).astype(np.float32)
        t_rec = time.perf_counter() - t0
    return 1e3 * t_model, 1e3 * t_rec


def measure(r, n, target, reps, with_numpy):
    import torch
    from plda_amd import MPlda, diarize
    dev = torch.device("cuda", 0)
    mean, T, psi = synthetic_model(D, 15)
    eng = MPlda(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    eng.set_model(mean, T, psi)
    vecs, _ = recordings(r, n, psi, 1000 * r + n)
    offsets = diarize.offsets_of([n] * r)
    block_off = diarize.offsets_of([n * n] * r)
    dX = torch.from_numpy(vecs).to(dev)
    S = torch.empty(r * n * n, dtype=torch.float32, device=dev)
    dims = torch.empty(r, dtype=torch.int32, device=dev)
    t, m = r * n, r * n - r
    labels, ncl = torch.empty(t, dtype=torch.int32, device=dev), torch.empty(r, dtype=torch.int32, device=dev)
    mg = (torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.int32, device=dev),
          torch.empty(m, dtype=torch.float64, device=dev))

    def score():
        eng.score_dense_pca_dev(dX.data_ptr(), offsets, target, S.data_ptr(), block_off, dims.data_ptr(), None)

    def score_ahc():
        eng.score_dense_pca_ahc_dev(dX.data_ptr(), offsets, target, 1, 0.0, None, labels.data_ptr(), ncl.data_ptr(), mg[0].data_ptr(),
                                    mg[1].data_ptr(), mg[2].data_ptr())

    def plain_ahc():
        eng.score_ahc_dev(dX.data_ptr(), offsets, 1, 0.0, None, labels.data_ptr(), ncl.data_ptr(), mg[0].data_ptr(), mg[1].data_ptr(),
                          mg[2].data_ptr())

    res = {"what": "dense PLDA scoring in every recording's PCA subspace, whole calls from HBM-resident rows",
           "host": socket.gethostname(), "R": r, "N": n, "D": D, "target_energy": target, "segments": t,
           "class": diarize.dense_pca_plan(eng, n, D)}
    res["score"] = _timed(score, reps)
    torch.cuda.synchronize()
    dd = dims.cpu().numpy()
    res["retained_dims"] = {"min": int(dd.min()), "median": float(np.median(dd)), "max": int(dd.max())}
    res["score_ahc"] = _timed(score_ahc, reps)
    res["plain_ahc_no_pca"] = _timed(plain_ahc, reps)
    res["clock_after"] = _clock()
    if with_numpy:
        count = min(r, max(1, 2000 // n))
        t_model, t_rec = numpy_call({"mean": mean, "transform": T, "psi": psi}, vecs, offsets, target, count)
        res["numpy_model_one_thread"] = {"numpy_recordings": count, "measured_ms": t_rec, "scaled_to_R_ms": t_rec * r / count,
                                         "model_covariances_ms": t_model, "numpy": np.__version__}
    del eng
    return res


def measure_parity():
    import dense_pca_model as dm
    from plda_amd import MPlda, diarize
    model, x, offsets, target = dm.ill_conditioned_case()
    s_eigh, d, lam = dm.score_block(model, x, target, "eigh")
    s_svd, _, lam_svd = dm.score_block(model, x, target, "svd")
    eng = MPlda(0)
    eng.set_model(model["mean"], model["transform"], model["psi"])
    (blk,), info = diarize.score_dense_pca(eng, x, offsets, target, return_info=True)
    return {"what": "ill-conditioned case (planted variances spanning 1e-6, target 0.99999): eigh / SVD spread of the model, "
                    "device deviation from the eigh route",
            "host": socket.gethostname(), "N": int(x.shape[0]), "D": int(x.shape[1]), "retained_dim": int(d),
            "device_dim": int(info["dims"][0]), "lam_over_lam1": (lam / lam[0]).tolist(),
            "block_spread_eigh_svd": float(np.abs(s_eigh - s_svd).max()),
            "block_device_minus_eigh": float(np.abs(blk.astype(np.float64) - s_eigh).max()),
            "block_fp32_half_ulp_at_max": float(2.0 ** -24 * np.abs(s_eigh).max()), "block_max_abs": float(np.abs(s_eigh).max()),
            "eig_spread_eigh_svd_over_lam1": float(np.abs(lam - lam_svd).max() / lam[0]),
            "eig_device_minus_eigh_over_lam1": float(np.abs(info["eigenvalues"][0] - lam).max() / lam[0]),
            "eig_device_relative_worst": float((np.abs(info["eigenvalues"][0] - lam_svd) / lam_svd).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="2000x100,200x1000,16x4096")
    ap.add_argument("--targets", default="0.1,0.5")
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("dense_pca_bench.py: no GPU -- these are measurements, there is nothing to fall back to")
    os.makedirs(args.outdir, exist_ok=True)

    def write(name, res):
        with open(os.path.join(args.outdir, name), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({k: res[k] for k in res if k not in ("what", "host")}), flush=True)

    if not args.no_parity:
        write("dense_pca_parity.json", measure_parity())
    for shape in args.shapes.split(","):
        r, n = (int(v) for v in shape.split("x"))
        for target in (float(v) for v in args.targets.split(",")):
            write("dense_pca_%dx%d_t%g.json" % (r, n, target), measure(r, n, target, args.reps, not args.no_numpy))


if __name__ == "__main__":
    main()
