"""GPU: a long-lived handle behaves like a fresh one.

The law (include/plda_hip.h, "a long-lived handle"): after ANY sequence of earlier successful or refused calls on a handle, a
call's outputs equal, bit for bit, the outputs of the same call on a fresh handle that holds the same model.  The poisoned-scratch
tests catch a read of memory nobody wrote (0xFF bytes show up as NaN); they run one call on a fresh handle and cannot catch a
read of memory an EARLIER, LARGER call wrote, or a cache that outlives what it was computed from: those values are finite and
plausible.  This file goes there.  The probes, the buffers they reach and the comparison live in tests/history_cases.py (held to
their own laws, and shown to be able to fail, by tests/test_history_cases.py); the comparison is np.array_equal on the uint8
views, so no tolerance is introduced here.

  (a) control            every probe on two fresh handles
  (b) shrink and regrow  large -> small -> large, small -> large -> small, and through the third probe of a family with classes
  (c) neighbours         for every buffer several modules share, every ordered pair of different modules: X, then Y equals fresh;
                         the solver chain and the grouping chain
  (d) model routes       every model-keyed cache warmed under one model, the model replaced by each route, every consumer again
  (e) after a refusal    documented refusals that come after device work began; the next valid calls equal fresh
  (f) a seeded walk      two handles with different models, 48 steps drawn from probes, routes, refusals and stream moves

Fresh results are computed once per (probe, model, creation-time switches) and kept for the module.  Hand runs with fresh walks:
PLDA_HISTORY_SEED=<seed> [PLDA_HISTORY_STEPS=<count>] pytest -m gpu tests/test_gpu_handle_history.py  (committed: seed 0, 48 steps).

Nothing here provokes a fault: every input sits in a buffer the test owns and only documented refusals are tried."""
import os

import numpy as np
import pytest

import history_cases as H

pytestmark = pytest.mark.gpu

SEED = int(os.environ.get("PLDA_HISTORY_SEED", "0"))
STEPS = int(os.environ.get("PLDA_HISTORY_STEPS", "48"))


def _make(**switches):
    """a fresh handle, made with every creation-time switch of the suite cleared around it but `switches`, which it remembers
    (history_cases.switches_of): its results are held to fresh handles made under the same switches"""
    from plda_amd import MPlda
    from test_gpu_sweep import SWITCHES
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    try:
        for k, v in switches.items():
            assert k in SWITCHES, k
            os.environ[k] = str(v)
        eng = MPlda(0)
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    eng.history_switches = tuple(sorted((k, str(v)) for k, v in switches.items()))
    return eng


@pytest.fixture(scope="module")
def harness():
    return H.Harness(_make)


def _guarded(run):
    """A device fault ends the file at once (test_gpu_sweep.py::_stop_on_a_device_fault): nothing more is started on a device
    that has faulted."""
    from test_gpu_sweep import _stop_on_a_device_fault
    try:
        run()
    except Exception as e:      # noqa: BLE001
        _stop_on_a_device_fault(repr(e))
        raise


# ------------------------------------------------------------------------------------------- (a) control
@pytest.mark.parametrize("name", sorted(H.PROBES))
def test_control(harness, name):
    """the probe on two fresh handles (its home model installed where it has one): a probe that fails here is a finding about
    determinism, not about history"""
    _guarded(lambda: harness.check(_make(**H.PROBES[name].switches), name, "control"))


# ------------------------------------------------------------------------------------------- (b) shrink and regrow
# every family on a default handle (a family whose probes need a switch: under it), and the trials GEMM's families again on
# handles made with the bf16x3 contraction and with the one-wave-per-SIMD arm
_REGROW = [(f, H.PROBES[H.FAMILIES[f]["large"]].switches) for f in sorted(H.FAMILIES)]
_REGROW += [(f, sw) for sw in (H.BF16X3, H.BT4) for f in ("score", "prepared", "asnorm", "topn")]


def _sw_id(sw):
    return "-".join("%s=%s" % kv for kv in sorted(sw.items())) or "default"


@pytest.mark.parametrize("family,switches", _REGROW, ids=["%s-%s" % (f, _sw_id(sw)) for f, sw in _REGROW])
def test_shrink_and_regrow(harness, family, switches):
    _guarded(lambda: harness.shrink_and_regrow(_make(**switches), family))


# ------------------------------------------------------------------------------------------- (c) neighbours
_PAIRS = H.neighbour_pairs()


@pytest.mark.parametrize("buf,x,y", _PAIRS, ids=["%s-%s-%s" % p for p in _PAIRS])
def test_neighbours(harness, buf, x, y):
    _guarded(lambda: harness.neighbours(_make(**H.UNDER.get(buf, {})), x, y))


def test_tile_tables_across_a_stream_move(harness):
    """The one-wave-per-SIMD kernel's queue counters are zeroed once, on the stream of the first launch, and its tile tables are
    built on the stream of the launch that needed them: eight grids on the handle's own stream, two on a side stream, the
    eight again (their tables partly evicted meanwhile), back on the own stream, each equal to fresh."""
    import torch

    def run():
        eng = _make(**H.BT4)
        side = torch.cuda.Stream(torch.device("cuda", 0))
        harness.check(eng, "bt4.large", "own stream")
        eng.synchronize()
        eng.set_stream(side.cuda_stream)
        try:
            harness.check(eng, "bt4.small", "side stream")
            harness.check(eng, "bt4.large", "side stream")
            eng.synchronize()
        finally:
            eng.set_stream(None)
        harness.check(eng, "bt4.small", "back on the own stream")
        harness.check(eng, "score.large", "back on the own stream")
        harness.check(eng, "bt4.large", "back on the own stream")
    _guarded(run)


# every fp64 solver caller after each other (linalg_part, eigdc, jac_work and its captured sweep graph, simdiag_state and its
# warm start), then the callers of the grouping (fit_sort, fit_offsets, fit_hist, fit_roww)
SOLVER_CHAIN = ("fit.large", "lda.large", "embed_fit.large", "sym_eig.large", "spd_inverse.large", "gemm_f64.large", "fit.small", "lda.small",
                "embed_fit.small", "sym_eig.small", "spd_inverse.small", "gemm_f64.small", "spd_inverse.third", "sym_eig.large", "fit.large")
GROUPING_CHAIN = ("fit.large", "groups.small", "lda.large", "embed_fit.small", "groups.large", "fit.small", "lda.small", "embed_fit.large",
                  "groups.small", "fit.large")


def _adapt_and_blend(harness, eng):
    """adapt_update and blend inside the solver chain: each replaces the model, the model it leaves is held to a fresh handle's
    (the same route from the same model) and a consumer runs on it"""
    for route in ("adapt_update", "blend"):
        harness.install(eng, "B33")
        fresh = _make()
        fresh.set_model(*H.model("B33"))
        for e in (eng, fresh):
            H.ROUTES[route][0](e)
        a, b = eng.get_model(), fresh.get_model()
        H.same_bits(a, b, "the model %s leaves" % route)
        harness.check_here(eng, "transform.small", "after %s" % route)


@pytest.mark.parametrize("chain", ["solvers", "grouping"])
def test_chains(harness, chain):
    def run():
        eng = _make()
        for i, name in enumerate(SOLVER_CHAIN if chain == "solvers" else GROUPING_CHAIN):
            harness.check(eng, name, "%s chain" % chain)
            if chain == "solvers" and i in (2, 8):
                _adapt_and_blend(harness, eng)
    _guarded(run)


# ------------------------------------------------------------------------------------------- (d) model routes x cached consumers
# under model D104: K4's padded transform (tf_pad), the one-trial host cache, the uniform coefficients at n = 1 then n = 7, the
# bucketed and the depth-2D tables (coef_cache), a prepared test side (kept prepared), the dense-PCA covariances (dp_model), a
# long trial list (pair_tab) and norm (zn_cpad)
CONSUMERS = ("transform.small", "one.small", "score.small", "prepared.small", "dense_pca.small", "pairs.long", "groups.small")


def _leave_a_record(eng):
    dout, din = eng.dims()
    eng.adapt_reset()
    eng.adapt_accumulate(H.rng_of("routes.record", din).standard_normal((din + 30, din)))


@pytest.mark.parametrize("route", sorted(H.ROUTES))
def test_model_routes(harness, route):
    """Every consumer after the route equals a fresh handle given get_model() through set_model.  The documented refusals are
    asserted as such: the adaptation record taken under the old model is refused by the update (PLDA_E_INVAL: another epoch),
    dense PCA on the truncated model is refused (PLDA_E_INVAL), and the accepted calls that follow still equal fresh.
    No route leaves bits that differ from set_model of the same numbers (the offset -T mean is recomputed by one kernel on
    every route), so every pair is compared bit for bit; set_model.same installs ANOTHER model of the warmed model's dimension."""
    def run():
        eng = _make()
        apply = H.ROUTES[route][0]
        truncated = route == "truncate"

        # why the update is refused: the record's epoch (after the adapt_update route, the epoch of the record that route took
        # and used); after truncate the model is not square, which is asked first
        why = "truncat" if truncated else "taken under an earlier model"

        def after(e):
            H.expect_status(e, H.E_INVAL, e.adapt_update, why)
            e.adapt_reset()
            if truncated:
                H.refuse_dense_truncated(e)

        consumers = [c for c in CONSUMERS if not (truncated and c.startswith("dense_pca"))]
        harness.route(eng, "D104", CONSUMERS, apply, consumers, _leave_a_record, after)
        if truncated:
            harness.check(eng, "dense_pca.small", "a square model after the truncated one")
        harness.check(eng, "adapt.small", "the adaptation record after the route")
    _guarded(run)


def test_lda_and_embedding_routes(harness, tmp_path):
    """The LDA model through lda_fit and lda_set_model (LDA.load), the embedding chain through embed_set, embed_fit and
    embed_clear: the model or chain installed last is the one in use, whatever was installed before."""
    def run():
        from plda_amd.lda import LDA
        used, fresh = _make(), _make()
        inp = H.PROBES["lda.small"].inputs()
        small = LDA("svd", engine=fresh)
        small.fit(inp["x"], inp["y"])
        path = str(tmp_path / "small.npz")
        small.save(path)
        want = dict(lp=small.predict_log_proba(inp["x"][:31]), tr=small.transform(inp["x"][:31]))
        harness.check(used, "lda.large", "before the loaded model")
        loaded = LDA(engine=used).load(path)
        H.same_bits(dict(lp=loaded.predict_log_proba(inp["x"][:31]), tr=loaded.transform(inp["x"][:31])), want, "a loaded LDA model after a larger fit")
        harness.check(used, "lda.small", "a fit after the loaded model")
        for name in ("embed.large", "embed_fit.large", "embed.small", "embed.centre", "embed_fit.small", "embed.third", "embed.large", "embed.centre"):
            harness.check(used, name, "embedding routes")
    _guarded(run)


# ------------------------------------------------------------------------------------------- (e) after a refused call
@pytest.mark.parametrize("name", sorted(H.REFUSALS))
def test_after_a_refused_call(harness, name):
    """the status code is asserted by the refusal itself (history_cases.expect_status); then the next valid call of the same
    module, and of one module that shares a buffer with it, equals fresh"""
    call, own, other, home = H.REFUSALS[name]
    _guarded(lambda: harness.after_refusal(_make(), home, call, own, other))


# ------------------------------------------------------------------------------------------- (f) a seeded walk
# the probes that run under whatever model the handle holds (every other one installs its home model first: dense PCA and the
# adaptation need a square model, and a probe without a model does not care)
ROAMING = tuple(n for n, p in sorted(H.PROBES.items()) if p.home is not None and p.module not in ("dense_pca", "adapt"))


def test_seeded_walk(harness):
    import torch
    steps = H.walk_steps(SEED, STEPS, H.WALK_PROBES, sorted(H.ROUTES), sorted(H.REFUSALS))
    print("PLDA_HISTORY_SEED=%d PLDA_HISTORY_STEPS=%d: %s" % (SEED, STEPS, steps))
    streams = {}

    def stream(eng, side):
        eng.synchronize()
        torch.cuda.synchronize()
        if side:
            streams[id(eng)] = torch.cuda.Stream(torch.device("cuda", 0))
            eng.set_stream(streams[id(eng)].cuda_stream)
        else:
            eng.set_stream(None)

    def run():
        engines = [_make(), _make()]
        engines[0].set_model(*H.model("D104"))
        engines[1].set_model(*H.model("B33"))
        try:
            harness.walk(engines, steps, H.ROUTES, H.REFUSALS, ROAMING, stream)
        finally:
            for e in engines:
                e.synchronize()
                e.set_stream(None)
    _guarded(run)
