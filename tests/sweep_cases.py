"""tests/sweep_cases.py -- seeded, edge-biased case generators of the parity sweep (tests/test_gpu_sweep.py runs the cases on
the device, tests/test_sweep_cases.py holds the generators to their own laws on the host).  NumPy only.

    draw(module, index, seed0=0) -> case     a dict; seeded by (module name, seed0, index) ALONE: case 17 of a module is the
                                             same object whatever else ran
    case["tag"]                              one line (module, index, seed0, shape, content, options), printed on failure;
                                             `draw(module, index, seed0)` re-creates the case from it
    case["hits"]                             {menu name: entry} -- which entry of every menu of MENUS[module] the case exercises
    case["redraws"]                          how often the draw was repeated (next sub-seed) because the module's own host
                                             model found it ill-posed
    COUNTS[module]                           the committed number of cases at seed0 = 0
    MENUS[module]                            {menu name: entries}: the smallest sizes at which the kernel's structure changes,
                                             the content kinds (tie-heavy and degenerate ones always among them), the forms and
                                             the dispatch classes; tests/test_sweep_cases.py asserts that the committed cases
                                             hit every entry

How an entry is chosen: indices are cut into blocks of len(menu); inside a block the menu is dealt out in an order seeded by
(module, seed0, menu name, block) -- so ANY len(menu) consecutive cases hit every entry, the pairing between menus is random,
and the choice still depends on (module, seed0, index) alone.  Everything else comes from the case's own generator.
"""
import zlib

import numpy as np

MODULES = ("topn", "der", "ahc", "asnorm", "mindcf", "calibration", "embed", "vbx", "adapt", "fusion", "transform")
COUNTS = {"topn": 24, "der": 24, "ahc": 24, "asnorm": 30, "mindcf": 24, "calibration": 30, "embed": 24, "vbx": 24, "adapt": 24, "fusion": 24,
          "transform": 24}
MAX_REDRAWS = 16


def _key(text):
    return zlib.crc32(text.encode())


def _rng(module, seed0, index, sub=0):
    return np.random.default_rng([_key(module), int(seed0), int(index), int(sub)])


class _Picker(object):
    """The menus of one case."""

    def __init__(self, module, seed0, index):
        self.module, self.seed0, self.index = module, int(seed0), int(index)
        self.hits = {}

    def __call__(self, name, index=None):
        menu = MENUS[self.module][name]
        block, pos = divmod(self.index if index is None else index, len(menu))
        order = np.random.default_rng([_key(self.module), self.seed0, _key(name), block]).permutation(len(menu))
        entry = menu[int(order[pos])]
        self.hits[name] = entry
        return entry

    def cycle(self, name):
        """(entry, rank): the menu dealt out in its written order, and how many earlier cases got the same entry -- the index
        under which such a case picks from the menus that only this entry uses, so that they too are covered block by block"""
        menu = MENUS[self.module][name]
        entry = self.hits[name] = menu[self.index % len(menu)]
        return entry, sum(1 for j in range(self.index) if menu[j % len(menu)] == entry)

    def rank_in(self, name, group):
        """how many earlier cases drew one of `group` from the cycled menu `name`"""
        menu = MENUS[self.module][name]
        return sum(1 for j in range(self.index) if menu[j % len(menu)] in group)

    def force(self, name, entry):
        assert entry in MENUS[self.module][name], (name, entry)
        self.hits[name] = entry
        return entry


class IllPosed(Exception):
    """Raised by a generator when the module's own host model finds the draw ill-posed; draw() takes the next sub-seed."""


def draw(module, index, seed0=0):
    for sub in range(MAX_REDRAWS):
        pick = _Picker(module, seed0, index)
        try:
            case = _GENERATORS[module](pick, _rng(module, seed0, index, sub))
        except IllPosed as e:
            why = str(e)
            continue
        case.update(module=module, index=int(index), seed0=int(seed0), redraws=sub, hits=dict(pick.hits))
        case["tag"] = "%s-%d seed0=%d%s: %s" % (module, index, seed0, " redraws=%d" % sub if sub else "", case.pop("what"))
        return case
    raise AssertionError("%s-%d seed0=%d: %d draws in a row were ill-posed (a generator bug): %s" % (module, index, seed0, MAX_REDRAWS, why))


def cases(module, seed0=0, count=None):
    return [draw(module, i, seed0) for i in range(COUNTS[module] if count is None else count)]


def _opts(**kw):
    return " ".join("%s=%s" % (k, v) for k, v in kw.items())


MENUS = {}
_GENERATORS = {}


# =========================================================================================== top-N (K12, csrc/topn.hip)
TOPN_MAX = 256
TOPN_CONTENTS = ("gaussian", "equal", "zeros", "ascending", "descending", "binade", "nonfinite", "duplicates")     # test_gpu_topn._content
TOPN_MODES = ("raw", "znorm", "snorm both", "snorm enrol", "snorm test")                                          # test_gpu_topn.MODES
MENUS["topn"] = {
    "m": (1, 2, 63, 64, 65, 127, 128, 129, 257),
    "nt": (1, 3, 4, 5, 63, 64, 65, 1000, 1023, 1025, 4097),
    "n0": (1, 2, 10, 100, 256, "length"),          # top_n along axis 0 (a line is a row), clipped to the line's length
    "n1": (1, 2, 10, 100, 256, "length"),          # ... along axis 1
    "ld": ("nt", "pad4+4", "nt+1"),
    "form": ("matrix", "matrix", "operand"),
    "content": TOPN_CONTENTS,                      # matrix form
    "mode": TOPN_MODES,                            # operand form
    "counts": ("uniform", "two", "big"),           # operand form: the three GEMM depths
    "d": (48, 200, 257),                           # operand form
}


def topn_n(entry, length):
    return min(TOPN_MAX, length) if entry == "length" else min(int(entry), length)


def _topn_operands(rng, d, kind, m, nt):
    """test_gpu_topn._operands with a generator of the case's own: a third of the test rows are copies of others, a third of
    the enrol rows are copies of others WITH their counts and statistics -- exact ties along both axes."""
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    if kind == "uniform":
        n = 3
    elif kind == "two":
        n = rng.choice(np.array([2, 5], np.int32), m).astype(np.int32)
    else:
        n = rng.choice(np.array([1, 3, 5000], np.int32), m).astype(np.int32)       # a count above 4095: the depth-2D form
    src_v, src_u = rng.integers(0, nt, nt // 3), rng.integers(0, m, m // 3)
    dst_v, dst_u = rng.permutation(nt)[:nt // 3], rng.permutation(m)[:m // 3]
    st = dict(zm=rng.standard_normal(m) * 10 - 20, zs=0.5 + 5 * rng.random(m), em=rng.standard_normal(m) * 10 - 20,
              es=0.5 + 5 * rng.random(m), tm=rng.standard_normal(nt) * 10 - 20, ts=0.5 + 5 * rng.random(nt))
    st["zs"][::7] = 0.0                       # a zero std leaves the row un-normalised
    st["es"][::11] = 0.0
    st["ts"][::5] = 0.0
    for dst, src in zip(dst_v, src_v):
        V[dst] = V[src]
        st["tm"][dst], st["ts"][dst] = st["tm"][src], st["ts"][src]
    for dst, src in zip(dst_u, src_u):
        U[dst] = U[src]
        if not np.isscalar(n):
            n[dst] = n[src]
        for k in ("zm", "zs", "em", "es"):
            st[k][dst] = st[k][src]
    if kind == "big":
        n[0] = 5000
    return U, n, V, st


def _draw_topn(pick, rng):
    from topn_model import content as _content
    m, nt, (form, rank) = pick("m"), pick("nt"), pick.cycle("form")
    n0, n1 = pick("n0"), pick("n1")
    # a top_n longer than the line: on even cases the line grows to the menu's next size that holds it, on odd ones the whole
    # line is asked for (an entry counts as hit only where it is what runs)
    if n0 != "length" and n0 > nt:
        if pick.index % 2 == 0:
            nt = pick.force("nt", min(v for v in MENUS["topn"]["nt"] if v >= n0))
        else:
            n0 = pick.force("n0", "length")
    if n1 != "length" and n1 > m:
        if pick.index % 2 == 0:
            m = pick.force("m", min(v for v in MENUS["topn"]["m"] if v >= n1))
        else:
            n1 = pick.force("n1", "length")
    if n0 == "length" and nt > TOPN_MAX:         # (top_n stops at 256: the whole of a longer line cannot be asked for)
        n0 = pick.force("n0", TOPN_MAX)
    if n1 == "length" and m > TOPN_MAX:
        n1 = pick.force("n1", TOPN_MAX)
    case = dict(m=m, nt=nt, form=form, top=(topn_n(n0, nt), topn_n(n1, m)))
    if form == "matrix":
        ldk, content = pick("ld", rank), pick("content", rank)
        case["ld"] = {"nt": nt, "pad4+4": (nt + 3) // 4 * 4 + 4, "nt+1": nt + 1}[ldk]
        case["S"] = _content(content, m, nt, rng)
        case["what"] = "%dx%d " % (m, nt) + _opts(form=form, ld=case["ld"], content=content, top=case["top"])
    else:
        d, kind, mode = pick("d", rank), pick("counts", rank), pick("mode", rank)
        case["d"], case["mode"] = d, mode
        case["U"], case["n"], case["V"], case["stats"] = _topn_operands(rng, d, kind, m, nt)
        case["model_seed"] = int(rng.integers(1 << 30))
        case["what"] = "%dx%d " % (m, nt) + _opts(form=form, D=d, counts=kind, mode=mode, top=case["top"])
    return case


_GENERATORS["topn"] = _draw_topn


def model_params(d, seed):
    """(mean, transform, psi) of a synthetic model, as tests/test_gpu_topn.py::_engine sets one."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    return rng.random(d), q * (1.0 + rng.random(d))[:, None], np.sort(0.05 + 4.0 * rng.random(d))[::-1].copy()


# =========================================================================================== DER (K17, csrc/der.hip)
DER_MAX_REF, DER_MAX_HYP = 64, 4096


def der_lds_max(sr):
    """The widest matrix of the LDS class at sr reference speakers: csrc/der.hip's der_lds_bytes restated (the device test
    asserts plda_der_plan's answer against it)."""
    fixed = 8 * (4 + 16 + 1 + 65 + 64) + 4 * (64 + 64 + 4)
    w = 1
    while w < DER_MAX_HYP and 8 * sr * (w + 1) + 32 * (w + 2) + fixed <= 160 * 1024:
        w += 1
    return w


MENUS["der"] = {
    "n": (1, 2, 5, 64, 65, 300),
    "sr": ("1", "mid", "max"),                     # distinct reference labels: 1, in between, min(64, N)
    "sh": ("1", "mid", "n"),                       # distinct hypothesis labels: 1, in between, N
    "nonspeech": ("none", "some", "all_but_one"),  # share of label -1 in the reference (the hypothesis: none / some)
    # ticks: NULL (ones), small with zeros, all equal (tie-heavy matrices), 2^31 - 1 everywhere: sums pass 2^32 from N = 5 on
    # and reach 300 (2^31 - 1) ~ 2^39.2 at the largest N of this menu (2^40 needs more than 512 segments: that stays with
    # test_gpu_der.py::test_sums_beyond_32_and_40_bits)
    "dur": ("null", "zeros", "equal", "huge"),
    "cls": ("lds", "lds", "lds", "lds", "lds", "lds", "lds", "scratch"),       # scratch: Sr = 64 and more than der_lds_max(64) hypothesis labels
    "form": ("der", "der", "sweep"),
    "records": (1, 3),
}


def _der_labels(rng, n, count, limit):
    """n labels holding exactly `count` distinct values of range(limit), the values with gaps"""
    vals = np.sort(rng.choice(limit, count, replace=False))
    lab = np.concatenate([np.arange(count), rng.integers(0, count, n - count)])
    rng.shuffle(lab)
    return vals[lab].astype(np.int32)


def _der_recording(rng, n, sr, sh, nonspeech, durk):
    ref, hyp = _der_labels(rng, n, sr, DER_MAX_REF), _der_labels(rng, n, sh, DER_MAX_HYP)
    if nonspeech == "some":
        ref[rng.random(n) < 0.2] = -1
        hyp[rng.random(n) < 0.2] = -1
    elif nonspeech == "all_but_one":
        keep = int(rng.integers(n))
        ref[np.arange(n) != keep] = -1
        hyp[rng.random(n) < 0.2] = -1
    if durk == "null":
        dur = None
    elif durk == "zeros":
        dur = rng.integers(0, 4, n).astype(np.int32)
    elif durk == "equal":
        dur = np.full(n, 3, np.int32)
    else:
        dur = np.full(n, 2 ** 31 - 1, np.int32)
        dur[rng.random(n) < 0.1] = 0
    return ref, hyp, dur


def _between(rng, lo, hi):
    return int(rng.integers(lo + 1, hi)) if hi - lo > 1 else (lo if rng.random() < 0.5 else hi)


def _draw_der(pick, rng):
    import ahc_model
    import der_model
    n, srk, nonspeech, durk, records = pick("n"), pick("sr"), pick("nonspeech"), pick("dur"), pick("records")
    (cls, _), (form, rank) = pick.cycle("cls"), pick.cycle("form")
    if cls == "scratch":
        n, form = pick.force("n", 300), pick.force("form", "der")
        srk, shk, nonspeech = pick.force("sr", "max"), pick.force("sh", "n"), pick.force("nonspeech", "none")
    elif form == "der":
        shk = pick("sh", rank)
    else:
        shk = "1"                                # (the sweep form makes its own hypothesis)
    sr = {"1": 1, "mid": _between(rng, 1, min(64, n)), "max": min(64, n)}[srk]
    sh = {"1": 1, "mid": _between(rng, 1, n), "n": n}[shk]
    first = _der_recording(rng, n, sr, sh, nonspeech, durk)
    recs = [first]
    for _ in range(records - 1):                 # the other recordings of the call: small, of the same dur kind
        k = int(rng.choice([1, 2, 5, 64, 65]))
        recs.append(_der_recording(rng, k, int(rng.integers(1, min(64, k) + 1)), int(rng.integers(1, k + 1)),
                                   str(rng.choice(["none", "some"])), durk))
    case = dict(form=form, ref=np.concatenate([r[0] for r in recs]), sizes=[len(r[0]) for r in recs],
                dur=None if durk == "null" else np.concatenate([r[2] for r in recs]))
    eff_sr, eff_sh = len(set(first[0][first[0] >= 0].tolist())), len(set(first[1][first[1] >= 0].tolist()))
    case["cls"] = int(max(eff_sr, eff_sh) > der_lds_max(eff_sr))
    case["shape"] = (eff_sr, eff_sh)
    if (cls == "scratch") != bool(case["cls"]):
        pick.force("cls", "scratch" if case["cls"] else "lds")
    if form == "der":
        case["hyp"] = np.concatenate([r[1] for r in recs])
    else:
        # the hypothesis of the sweep form is the cut of a drawn AHC merge record (the host model's, of drawn score blocks:
        # planted speakers under noise, or integer scores whose costs tie) at thresholds taken from that record
        blocks = []
        for k in case["sizes"]:
            if rng.random() < 0.5:
                sizes = np.bincount(rng.integers(0, max(1, min(4, k)), k))
                blocks.append(der_model.planted_block(sizes[sizes > 0], int(rng.integers(1 << 30)), noise=0.6)[0])
            else:
                blocks.append(ahc_model.integers(k, int(rng.integers(1 << 30))))
        full = ahc_model.cluster(blocks, None, 1)
        case["blocks"], case["merges"] = blocks, full[2:]
        cost = np.sort(full[4])
        if len(cost):
            at = cost[rng.integers(0, len(cost), 3)]
            thr = [-at[0], np.nextafter(-at[1], np.inf), np.nextafter(-at[2], -np.inf), -cost[-1] - 1.0, -cost[0] + 1.0, 0.0, -at[0]]
        else:
            thr = [0.0, 1.0]
        case["thresholds"] = np.asarray(thr, np.float64)
        case["num_speakers"] = None if rng.random() < 0.5 else [int(rng.integers(1, k + 1)) for k in case["sizes"]]
    case["what"] = "N=%s Sr x Sh=%dx%d " % (case["sizes"], eff_sr, eff_sh) + _opts(form=form, nonspeech=nonspeech, dur=durk, cls=case["cls"])
    return case


_GENERATORS["der"] = _draw_der


# =========================================================================================== AHC (K15, csrc/ahc.hip)
def ahc_lds_max():
    """csrc/ahc.hip's ahc_lds_max_calc() restated: 8 n (n - 1) / 2 + 28 n + 512 <= 160 KiB (the device test asserts
    plan()["lds_max"] against it)"""
    n = 1
    while 8 * (n + 1) * n // 2 + 28 * (n + 1) + 512 <= 160 * 1024:
        n += 1
    return n


AHC_LDS_MAX = ahc_lds_max()
AHC_FAMILIES = ("gaussian", "integers", "chain", "chain_reverse", "equal", "zeros")        # test_gpu_ahc.FAMILIES
MENUS["ahc"] = {
    "n": (1, 2, 3, 4, 63, 64, 65, AHC_LDS_MAX - 1, AHC_LDS_MAX, AHC_LDS_MAX + 1, 257),
    "records": (1, 2, 4, 8),
    "family": AHC_FAMILIES,
    # a threshold exactly at a merge cost of the model's record, one ulp above it, one ulp below it; a speaker count; both
    "stop": ("at", "above", "below", "num_speakers", "both"),
    "form": ("matrix", "matrix", "operand"),
    "d": (8, 200),                                 # operand form
}


def _ahc_block(family, n, rng):
    import ahc_model
    seed = int(rng.integers(1 << 30))
    if family in ("gaussian", "integers", "zeros"):
        return getattr(ahc_model, {"zeros": "signed_zeros"}.get(family, family))(n, seed)
    if family == "equal":
        return ahc_model.all_equal(n)
    return ahc_model.chain(n, family == "chain_reverse")


def ahc_stop(case, first_record):
    """(threshold, num_speakers) of a case from the model's FULL merge costs of its first recording."""
    cost = np.asarray(first_record, np.float64)
    cost = cost[np.isfinite(cost)]
    stop, u = case["stop"], case["stop_u"]
    thr = None
    if stop != "num_speakers":
        c = cost[int(u * len(cost))] if len(cost) else np.float64(0.0)
        thr = {"at": -c, "both": -c, "above": np.nextafter(-c, np.inf), "below": np.nextafter(-c, -np.inf)}[stop]
        thr = float(thr)
    return thr, (case["num_speakers"] if stop in ("num_speakers", "both") else None)


def _draw_ahc(pick, rng):
    n, records, stop, (form, rank) = pick("n"), pick("records"), pick("stop"), pick.cycle("form")
    sizes = [n] + [int(rng.choice([1, 2, 3, 4, 63, 64, 65, AHC_LDS_MAX + 1])) for _ in range(records - 1)]
    if records > 1 and n <= AHC_LDS_MAX and rng.random() < 0.5:
        sizes[-1] = AHC_LDS_MAX + 1              # a call of mixed classes
    case = dict(sizes=sizes, stop=stop, stop_u=float(rng.random()), form=form,
                num_speakers=[int(rng.integers(1, k + 1)) for k in sizes])
    if form == "matrix":
        fams = [pick("family", rank)] + [str(rng.choice(AHC_FAMILIES)) for _ in sizes[1:]]
        case["blocks"] = [_ahc_block(f, k, rng) for f, k in zip(fams, sizes)]
        case["what"] = "N=%s " % sizes + _opts(form=form, families=",".join(fams), stop=stop, u="%.3f" % case["stop_u"])
    else:
        d = pick("d", rank)
        spk = rng.standard_normal((6, d)) * 1.5
        case["d"], case["model_seed"] = d, int(rng.integers(1 << 30))
        case["vecs"] = np.concatenate([spk[rng.integers(0, 6, k)] + rng.standard_normal((k, d)) for k in sizes])
        case["what"] = "N=%s " % sizes + _opts(form=form, D=d, stop=stop, u="%.3f" % case["stop_u"])
    return case


_GENERATORS["ahc"] = _draw_ahc


# =========================================================================================== AS-norm cohort statistics (K9, csrc/snorm.hip)
# one 1024-thread workgroup per row; 16 wave shares of quads; radix levels of 11 / 11 / 10 bits; a compaction gate of 8192
# candidates; a per-wave cap of 1024
MENUS["asnorm"] = {
    "nc": (1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4097, 16385, 20011),
    "k": (1, 2, 300, 8192, 8193, "nc/2", "nc-1", "nc"),
    "r": (1, 3, 130),
    # ties and all-equal rows are made by REPEATING cohort rows (identical operands give bit-identical scores); `ordered`
    # puts the cohort rows closest to every test row side by side, so that one wave's share holds all the candidates
    "content": ("gaussian", "tripled", "identical", "ordered"),
    "counts": ("uniform", "two", "big"),
    "d": (48, 200),
}


def asnorm_k(entry, nc):
    k = {"nc/2": nc // 2, "nc-1": nc - 1, "nc": nc}.get(entry, entry)
    return max(1, min(int(k), nc))


ASNORM_NEAR = 2600         # `ordered`: that many cohort rows next to every test row, side by side from column 0


def _draw_asnorm(pick, rng):
    r, kind, d = pick("r"), pick("counts"), pick("d")
    content, rank = pick.cycle("content")
    if content != "ordered":                     # (the size menus are dealt over the cases that draw from them)
        others = pick.rank_in("content", [c for c in MENUS["asnorm"]["content"] if c != "ordered"])
        nc, ke = pick("nc", others), pick("k", others)
    else:
        # the cap overflow needs more than 1024 candidates in one wave's share (a 16th of the row: Nc > 16384) while all the
        # candidates number at most 8192: the two largest cohorts, K = 300 among 2600 near rows that fill the first shares
        nc, ke = pick.force("nc", (16385, 20011)[rank % 2]), pick.force("k", 300)
    if isinstance(ke, int) and ke > nc:          # a K the cohort cannot hold: the cohort grows on even cases, K is clipped on odd ones
        if pick.index % 2 == 0:
            nc = pick.force("nc", min(v for v in MENUS["asnorm"]["nc"] if v >= ke))
        else:
            ke = pick.force("k", "nc")
    X, Cv = rng.standard_normal((r, d)), rng.standard_normal((nc, d))
    if content == "tripled":                     # every cohort vector about three times: ties at every boundary
        Cv = Cv[rng.integers(0, max(1, nc // 3), nc)]
    elif content == "identical":                 # all scores of a row equal: std exactly 0 for every K
        Cv = np.repeat(Cv[:1], nc, axis=0)
    elif content == "ordered":
        x0 = rng.standard_normal(d)
        near = ASNORM_NEAR
        X = x0 + 0.05 * rng.standard_normal((r, d))
        Cv = np.concatenate([x0 + 0.05 * rng.standard_normal((near, d)), rng.standard_normal((nc - near, d))])
    if kind == "uniform":
        n = 3
    elif kind == "two":
        n = rng.choice(np.array([2, 5], np.int32), r).astype(np.int32)
    else:
        n = rng.choice(np.array([1, 3, 5000], np.int32), r).astype(np.int32)       # a count above 4095: the depth-2D form
        n[0] = 5000
    case = dict(d=d, X=X, Cv=Cv, n=n, K=asnorm_k(ke, nc), model_seed=int(rng.integers(1 << 30)))
    case["what"] = "Nc=%d K=%d R=%d D=%d " % (nc, case["K"], r, d) + _opts(content=content, counts=kind)
    return case


_GENERATORS["asnorm"] = _draw_asnorm


# =========================================================================================== the labelled-trials consumers
# (csrc/trial_source.hpp: strips of 1024 columns, 4 per thread, row slices; 16-byte loads only when ld % 4 == 0, the base is
# 16-byte aligned and the thread's fourth column exists) -- the EER, the minDCF, the calibration pass and fit, the fusion
TRIALS_MENUS = {
    "m": (1, 2, 3, 5, 37, 64, 129, 257),
    "nt": (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049),
    "ld": ("nt", "pad4+4", "nt+1"),
    "off": (0, 1),                                 # the base pointer that many floats off a 16-byte boundary
    "layout": ("one_target", "one_nontarget", "sqrt", "one_speaker"),
    "content": ("gaussian", "ties8", "separable", "inverted", "one_value", "zeros_mix"),
    # 16-byte loads (ld % 4 == 0, an aligned base, four columns) or 4-byte ones: what ld, off and nt amount to
    "loads": ("vector", "scalar"),
    # the operand form (rule B): slabs of 256 rows (csrc/operand_slabs.hip rounds PLDA_EER_SLAB_ROWS up to whole 256-row
    # tiles) and M above them -- 257: a last slab of one row, 513: two full slabs and one row --, each with and without
    # z-norm statistics (sliced per slab); the three GEMM depths
    "operand": ((257, False), (257, True), (513, False), (513, True)),
    "counts": ("uniform", "bucketed", "depth2d"),
}
OPERAND_SLAB_ROWS = 256


def trials_ld(kind, nt):
    return {"nt": nt, "pad4+4": (nt + 3) // 4 * 4 + 4, "nt+1": nt + 1}[kind]


def trials_labels(rng, m, nt, layout):
    """(enrol speakers, test speakers) int64 with at least one target and one non-target trial (m * nt >= 2)"""
    assert m * nt >= 2
    if layout == "one_target":
        es, ts = np.arange(m) + 1000, np.arange(nt) + 50000
        es[rng.integers(m)] = ts[rng.integers(nt)] = 7
    elif layout == "one_nontarget":
        es, ts = np.zeros(m, np.int64), np.zeros(nt, np.int64)
        if nt > 1:
            ts[rng.integers(nt)] = 3
        else:
            es[rng.integers(m)] = 3
    else:
        k = 1 if layout == "one_speaker" else max(2, int(round(np.sqrt(m))))
        es = rng.integers(0, k, m)
        ts = rng.integers(0, max(k, 2), nt)          # (one_speaker: every ROW is speaker 0, the columns are 0 or 1)
        tgt = es[:, None] == ts[None, :]
        if not tgt.any():
            ts[0] = es[0]
        if tgt.all() or (layout == "one_speaker" and (ts == 0).all()):
            if nt > 1:
                ts[-1] = 99
            else:
                es[-1] = 99
    es, ts = es.astype(np.int64), ts.astype(np.int64)
    tgt = es[:, None] == ts[None, :]
    assert tgt.any() and not tgt.all()
    return es, ts


def trials_scores(rng, m, ld, nt, tgt, content):
    """fp32 [m, ld] with the matrix in its first nt columns (the padding holds scores of the same law: never read)"""
    t = np.zeros((m, ld), bool)
    t[:, :nt] = tgt
    s = rng.standard_normal((m, ld))
    if content in ("gaussian", "ties8", "zeros_mix"):
        s = s + 2.0 * t
    elif content == "separable":
        s = np.clip(s, -3, 3) + 9.0 * t
    elif content == "inverted":
        s = s - 2.0 * t
    elif content == "one_value":
        s = np.full((m, ld), 1.25)
    s = s.astype(np.float32)
    if content == "ties8":                       # scores quantised to 8 values
        s = np.clip(np.round(s), -3, 4).astype(np.float32)
    if content == "zeros_mix":                   # -0.0 and +0.0 are ONE score
        s = np.round(s).astype(np.float32)
        z = s == 0
        s[z] = np.where(rng.random(int(z.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    return s


def _trials_shape(pick, rank):
    m, nt = pick("m", rank), pick("nt", rank)
    if m * nt < 2:                               # one trial cannot hold both classes
        if rank % 2:
            nt = pick.force("nt", 2)
        else:
            m = pick.force("m", 2)
    return m, nt


def _trials_operands(pick, rng, rank, d=48, speakers=30):
    """the operands of rule B: more rows than a slab of 256, speaker structure, counts of the three GEMM depths, z-norm
    statistics or none"""
    (m, zn), nt = pick("operand", rank), pick("nt", rank)
    if nt < 2:
        nt = pick.force("nt", 2)
    kind = pick("counts", rank)
    spk = rng.standard_normal((speakers, d)) * 1.5
    es, ts = rng.integers(0, speakers, m), rng.integers(0, speakers, nt)
    ts[0] = es[0]
    ts[-1] = speakers                            # a speaker nobody enrolled: at least one non-target
    U = spk[es] + rng.standard_normal((m, d))
    V = np.concatenate([spk, np.zeros((1, d))])[ts] + rng.standard_normal((nt, d))
    if kind == "uniform":
        n = 2
    elif kind == "bucketed":
        n = rng.integers(1, 4, m).astype(np.int32)
    else:
        n = rng.choice(np.array([1, 3, 5000], np.int32), m).astype(np.int32)       # a count above 4095: the depth-2D form
        n[0] = 5000
    z = (rng.standard_normal(m), 0.5 + rng.random(m)) if zn else None
    case = dict(d=d, m=m, nt=nt, U=U, V=V, n=n, z=z, es=es.astype(np.int64), ts=ts.astype(np.int64), model_seed=int(rng.integers(1 << 30)))
    return case, "%dx%d " % (m, nt) + _opts(form="operand", D=d, counts=kind, znorm=zn)


def _trials_matrix(pick, rng, rank, matrix_rank, content_menu="content", min_trials=2):
    """rank: among the cases of this form (the menus only this form uses); matrix_rank: among the cases of every matrix form
    (the shape menus, which the operand form does not use)"""
    m, nt = _trials_shape(pick, matrix_rank)
    if m * nt < min_trials:                      # too few trials for this form: the matrix grows to the menus' next sizes that hold them
        widths = MENUS[pick.module]["nt"]
        if m * max(widths) < min_trials:
            m = pick.force("m", min(v for v in MENUS[pick.module]["m"] if v * max(widths) >= min_trials))
        nt = pick.force("nt", min(v for v in widths if m * v >= min_trials))
    ldk, off, layout, content = pick("ld", matrix_rank), pick("off", matrix_rank), pick("layout", matrix_rank), pick(content_menu, rank)
    ld = trials_ld(ldk, nt)
    es, ts = trials_labels(rng, m, nt, layout)
    S = trials_scores(rng, m, ld, nt, es[:, None] == ts[None, :], content)
    loads = pick.force("loads", "vector" if ld % 4 == 0 and off == 0 and nt >= 4 else "scalar")
    case = dict(m=m, nt=nt, ld=ld, off=off, es=es, ts=ts, S=S, content=content)
    return case, "%dx%d " % (m, nt) + _opts(ld=ld, off=off, loads=loads, layout=layout, content=content)


# ------------------------------------------------------------------------------------------- minDCF and EER (K11, csrc/dcf.hip, csrc/eer.hip)
MENUS["mindcf"] = dict(TRIALS_MENUS, form=("matrix", "matrix", "operand"), points=("five", "nist"))


def _draw_mindcf(pick, rng):
    (form, rank), points = pick.cycle("form"), pick("points")
    if form == "matrix":
        case, what = _trials_matrix(pick, rng, rank, rank)
    else:
        case, what = _trials_operands(pick, rng, rank)
    case.update(form=form, points=points, what=what + " form=%s points=%s" % (form, points))
    return case


_GENERATORS["mindcf"] = _draw_mindcf


# ------------------------------------------------------------------------------------------- calibration (K10, csrc/calib.hip)
FIT_CONTENTS = ("gaussian", "ties8", "inverted", "zeros_mix")     # the kinds with a finite optimum (the others are the pass's)
MENUS["calibration"] = dict(TRIALS_MENUS, form=("pass", "fit", "operand"), fit_content=FIT_CONTENTS,
                            point=("start", "identity", "saturating", "drawn"),       # (a, c) of the pass, as test_gpu_calibration._points
                            theta=("fixed", "a_score"),                              # the threshold of the pass's miss / fa counts
                            prior=(0.5, 0.05),
                            shift=("0", "+k", "-k", "+100k", "-100k"))               # equivariance: scores k * s + d, k = 2^-10 .. 2^10


def _pass_point(pick, rng, rank, S):
    kind, thk = pick("point", rank), pick("theta", rank)
    smax = float(np.abs(S).max())
    a, c = {"start": (0.0, 0.0), "identity": (1.0, 0.0), "saturating": (300.0 / max(smax, 1e-30), 5.0),
            "drawn": (float(rng.uniform(0.1, 3.0)), float(rng.uniform(-3.0, 3.0)))}[kind]
    theta = 0.7 if thk == "fixed" else float(S.ravel()[rng.integers(S.size)])
    return (a, c, theta), _opts(point=kind, theta=thk)


def shifted(scores, k, d):
    return (k * np.asarray(scores, np.float32).astype(np.float64) + d).astype(np.float32)


def _fit_options(pick, rng, rank):
    prior, shift = pick("prior", rank), pick("shift", rank)
    k = 2.0 ** int(rng.integers(-10, 11))
    d = {"0": 0.0, "+k": k, "-k": -k, "+100k": 100.0 * k, "-100k": -100.0 * k}[shift]
    return prior, k, d, _opts(prior=prior, k="2^%d" % int(np.log2(k)), d=shift)


def _draw_calibration(pick, rng):
    import calibration_model as cm
    form, rank = pick.cycle("form")
    if form == "operand":
        case, what = _trials_operands(pick, rng, rank)
        case["passes"] = [(1.0, 0.0, 0.0), (float(rng.uniform(0.1, 3.0)), float(rng.uniform(-3.0, 3.0)), float(rng.uniform(-2.0, 5.0)))]
    elif form == "pass":
        case, what = _trials_matrix(pick, rng, rank, pick.rank_in("form", ("pass", "fit")))
        pt, more = _pass_point(pick, rng, rank, case["S"][:, :case["nt"]])
        case["passes"], what = [pt], what + " " + more
    else:
        # (a fit of a handful of trials has no finite optimum: the row grows to the menu's next width that holds 64 trials)
        case, what = _trials_matrix(pick, rng, rank, pick.rank_in("form", ("pass", "fit")), "fit_content", min_trials=64)
        prior, k, d, more = _fit_options(pick, rng, rank)
        pos, neg = cm.split(case["S"][:, :case["nt"]], case["es"], case["ts"])
        try:
            f = cm.fit(pos, neg, prior)
            f2 = cm.fit(shifted(pos, k, d), shifted(neg, k, d), prior)
        except ValueError as e:
            raise IllPosed(str(e))
        if not (f["converged"] and f2["converged"]) or f["separable"] or f2["separable"] or not cm.equivariant(f["a"], f["b"], f2["a"], f2["b"], k, d):
            raise IllPosed("conv %s %s sep %s %s eq %s a %g %g b %g %g" % (f["converged"], f2["converged"], f["separable"], f2["separable"],
                                                                          cm.equivariant(f["a"], f["b"], f2["a"], f2["b"], k, d), f["a"], f2["a"] * k, f["b"], f2["b"] + f["a"] * d / k))
        # the rule's clause cllr_after <= min(1, cllr_before) is a law at prior 0.5 only (there the fit minimises Cllr itself):
        # off it, a lopsided set's optimum can sit above 1 (test_gpu_calibration.test_fit_off_prior_half_on_a_lopsided_set);
        # such a draw says nothing about the device
        if not f["cllr_after"] <= min(1.0, f["cllr_before"]):
            raise IllPosed("the model's own Cllr after the fit is %.4f" % f["cllr_after"])
        case.update(prior=prior, k=k, d=d)
        what += " " + more
    case.update(form=form, what=what + " form=" + form)
    return case


_GENERATORS["calibration"] = _draw_calibration


# =========================================================================================== embedding chain (K18, csrc/embed.hip)
EMBED_FORMS = ("kaldi", "vbx", "centre", "bare_A", "A_mout", "len_in_only")       # test_embed_model.FORMS
MENUS["embed"] = {
    # test_gpu_embed.PAIRS and four more: Din below, at and across the 16-deep stage and the 64 / 256 edges; Dout on either side of 512
    "pair": ((1, 1), (7, 15), (16, 16), (17, 17), (17, 1), (200, 150), (256, 200), (520, 512), (520, 513), (3, 2), (65, 64), (257, 130)),
    "dtype": ("float32", "float64"),
    "r": (1, 2, 15, 16, 17, 63, 64, 65, 129),
    "form": EMBED_FORMS,
    "offset": (0.0, 1e5),
    "cls": ("natural", "natural", "forced"),       # forced: class 2 under PLDA_EMBED_VARIANT=1 (the forms with a matrix)
}


def _draw_embed(pick, rng):
    from test_embed_model import make_chain
    (din, dout), dt, r, offset = pick("pair"), pick("dtype"), pick("r"), pick("offset")
    cls, rank = pick.cycle("cls")
    form = pick("form", rank)
    if cls == "forced" and form in ("centre", "len_in_only"):        # no matrix, nothing to force: the case runs in its own class
        cls = pick.force("cls", "natural")
    ch = make_chain(form, din, dout, rng, offset)
    x = (rng.standard_normal((r, din)) + offset).astype(dt)
    want_cls = 0 if ch.A is None else 2 if (cls == "forced" or dout > 512) else 1
    case = dict(din=din, dout=dout, chain=ch, x=x, forced=cls == "forced", cls=want_cls,
                chain_parts=[a for a in (ch.m_in, ch.A, ch.m_out) if a is not None])
    case["what"] = "%d->%d R=%d " % (din, dout, r) + _opts(form=form, dtype=dt, offset=offset, cls=want_cls, forced=cls == "forced")
    return case


_GENERATORS["embed"] = _draw_embed


# =========================================================================================== VBx (K16, csrc/vbx.hip)
VBX_LOOP = (0.0, 0.65, 0.9, 0.99)
MENUS["vbx"] = {
    "t": (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 130, 257),       # every residue mod 4 and mod 8: the chain prefetches 4 or 8 rows
    "d": (1, 2, 3, 7, 16, 33, 64, 65, 130),
    "s": (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 64),                # a row takes the power of two >= S lanes
    "loop_prob": VBX_LOOP,
    "params": ("default", "mid", "unit"),                      # (Fa, Fb) of vbx_model.PARAMS
    "records": (1, 2, 6),
    "empty": (False, True),                                    # label values with no segment
    "cls": ("lds", "lds", "lds", "hbm"),                       # hbm: 3 T S + ... above vbx_model.LDS_DOUBLES
}


def _vbx_recording(rng, t, d, k, s, phi, empty):
    import vbx_model
    y, labels, _, _ = vbx_model.generate(t, d, k, s, int(rng.integers(1 << 30)))
    # (generate returns its own phi: the same formula, a function of d alone)
    if empty and s >= 3:
        gone = int(rng.integers(0, s - 1))       # a label value below the largest that no segment carries
        labels = np.where(labels == gone, s - 1, labels).astype(np.int32)
    return y, labels


def _draw_vbx(pick, rng):
    import vbx_model as M
    t, d, s, p, pset, records, empty = pick("t"), pick("d"), pick("s"), pick("loop_prob"), pick("params"), pick("records"), pick("empty")
    if empty and s < 3:
        empty = pick.force("empty", False)
    cls, _ = pick.cycle("cls")
    phi = 30.0 * np.exp(-4.0 * np.arange(d) / d)
    fa, fb, _ = M.PARAMS[pset]
    shapes = [(t, s)]
    for _ in range(records - 1):                 # the other recordings of the call: the LDS buckets, and one of the HBM class
        shapes.append((int(rng.choice(MENUS["vbx"]["t"][:-1])), int(rng.choice(MENUS["vbx"]["s"]))))
    if cls == "hbm" or records == 6:             # a recording of the HBM class beside whatever the menus drew
        shapes.append((130, 64) if pick.index % 8 < 4 else (257, 33))
    recs, refs = [], []
    kw = dict(fa=fa, fb=fb, loop_prob=p, max_iters=M.ITERS, epsilon=-np.inf)
    for tt, ss in shapes:
        y, labels = _vbx_recording(rng, tt, d, max(1, min(4, ss)), ss, phi, empty)
        a, b = M.run(y, labels, phi, dtype=np.float64, **kw), M.run(y, labels, phi, dtype=np.longdouble, **kw)
        # what makes `labels must EQUAL the model's` and the parity band well-posed: the conditions of
        # tests/test_vbx_model.py::test_conditions_of_the_gpu_cases
        ok = (M.margin(a["gamma"]) >= 1e-6 and np.array_equal(a["labels"], b["labels"]) and a["n_clusters"] == b["n_clusters"]
              and np.isfinite(a["elbo"]).all() and np.isfinite(np.asarray(b["elbo"], np.float64)).all()
              and a["iters"] == M.ITERS and max(M.deviation(a, b)) <= 1e-9)
        if not ok:
            raise IllPosed("T=%d S=%d: margin %.3g" % (tt, ss, M.margin(a["gamma"])))
        recs.append((y, labels))
        refs.append((a, b))
    real = [int(M.state_doubles(len(l), int(l.max()) + 1, d) > M.LDS_DOUBLES) for _, l in recs]
    pick.force("cls", "hbm" if max(real) else "lds")
    case = dict(d=d, phi=phi, params=(fa, fb, p), recs=recs, refs=refs, classes=real)
    case["what"] = "TxS=%s D=%d " % ([(len(l), int(l.max()) + 1) for _, l in recs], d) + _opts(params=pset, loop_prob=p, empty=empty, classes=real)
    return case


_GENERATORS["vbx"] = _draw_vbx


# =========================================================================================== adaptation (K14, csrc/adapt.hip)
ADAPT_SCALES = (0.0, 0.3, 0.7, 1.0)
MENUS["adapt"] = {
    # 1: the smallest dimension a model has; both sides of the 64-wide tile; 208 / 209: the single-workgroup SYRK limit (the
    # augmented slab is D + 1 wide)
    "d": (1, 2, 3, 8, 24, 63, 64, 65, 200, 208, 209, 257),
    "n": ("1", "2", "D-1", "D", "D+1", "3D+50"),
    "weights": ("none", "random", "zeros"),
    "offset": (0.0, 0.3, 1e3),                     # of the data from the model mean, in within-class standard deviations
    "ws": ADAPT_SCALES, "bs": ADAPT_SCALES, "mds": ADAPT_SCALES,
    "alpha": (0.0, 0.25, 1.0), "alpha_mean": (0.0, 0.25, 1.0),
}


def _draw_adapt(pick, rng):
    import adapt_model as AM
    _assert_model = AM.assert_model
    d, nk, wk, offset = pick("d"), pick("n"), pick("weights"), pick("offset")
    # (10^3 standard deviations off the mean, any mean_diff_scale > 0 puts a rank-one term 10^6 times the model's covariance
    # into the update, and the model's own two restatements of it differ by more than the band: the scale is 0 there, where
    # the device has to cancel that term exactly)
    scales = (pick("ws"), pick("bs"), pick.force("mds", 0.0) if offset == 1e3 else pick("mds"))
    alpha, alpha_mean = pick("alpha"), pick("alpha_mean")
    n = max(1, {"1": 1, "2": 2, "D-1": d - 1, "D": d, "D+1": d + 1, "3D+50": 3 * d + 50}[nk])
    model = AM.synthetic_model(d, int(rng.integers(1 << 30)))
    other = AM.synthetic_model(d, int(rng.integers(1 << 30)))
    mean, T, psi = model
    W, _ = AM.covariances(T, psi)
    shift = offset * np.sqrt(np.diag(W)) * rng.choice([-1.0, 1.0], d)
    x = AM.sample(mean, T, psi, n, int(rng.integers(1 << 30)), scale=float(rng.choice([0.5, 1.5])), offset=shift)
    w = None
    if wk != "none":
        w = rng.random(n) + 0.05
        if wk == "zeros":
            w = w * (rng.random(n) < 0.6)
            w[int(rng.integers(n))] = 0.75       # (a record of total weight 0 is refused: one row keeps its weight)
    rec = AM.record(x, mean, w)
    ref = AM.update_kaldi(mean, T, psi, rec, *scales)
    try:                                         # the two restatements of the update agree where the update is well-posed
        _assert_model(AM.update_short(mean, T, psi, rec, *scales), ref)
        if not (np.isfinite(ref["psi"]).all() and np.isfinite(ref["transform"]).all()):
            raise IllPosed("the model's update is not finite")
    except (AssertionError, np.linalg.LinAlgError) as e:
        raise IllPosed("the two forms of the update differ: %s" % str(e)[:80])
    cut = sorted(int(v) for v in rng.integers(0, n + 1, 2))
    case = dict(d=d, model=model, other=other, x=x, w=w, scales=scales, alpha=alpha, alpha_mean=alpha_mean, pieces=[0] + cut + [n])
    case["what"] = "D=%d N=%d " % (d, n) + _opts(weights=wk, offset=offset, scales=scales, alpha=alpha, alpha_mean=alpha_mean)
    return case


_GENERATORS["adapt"] = _draw_adapt


# ------------------------------------------------------------------------------------------- fusion (K13, csrc/fusion.hip)
FUSION_UNITS = (1.0, 2.5, 0.4, 1.0, 1.5, 0.7, 2.0, 1.2)          # every system in its own units (test_gpu_fusion._systems)
MENUS["fusion"] = {k: v for k, v in TRIALS_MENUS.items() if k not in ("operand", "counts")}
MENUS["fusion"].update(form=("pass", "pass", "fit"), fit_content=FIT_CONTENTS, k=(1, 2, 3, 4, 5, 6, 7, 8),
                       point=("start", "alone", "cancel", "drawn"),                # (a, c) of the pass, as test_gpu_fusion._points
                       prior=(0.5, 0.05))
FUSION_FIT_TRIALS = 150000       # K x trials above which the host model's fit runs for more than a few seconds


def _draw_fusion(pick, rng):
    import fusion_model as fm
    (form, rank), k = pick.cycle("form"), pick("k")
    case, what = _trials_matrix(pick, rng, rank, pick.index, "content" if form == "pass" else "fit_content", 2 if form == "pass" else 400 * k)
    if form == "fit" and pick.hits["layout"] in ("one_target", "one_nontarget"):      # (one trial of a class is separable in K dimensions)
        pick.force("layout", "sqrt")
        case["es"], case["ts"] = trials_labels(rng, case["m"], case["nt"], "sqrt")
        what = what.replace("layout=one_target", "layout=sqrt").replace("layout=one_nontarget", "layout=sqrt")
    m, nt = case["m"], case["nt"]
    if form == "fit" and k * m * nt > FUSION_FIT_TRIALS:             # the row shrinks to the menu's widest that the model fits in seconds
        nt = case["nt"] = pick.force("nt", max(v for v in MENUS["fusion"]["nt"] if k * m * v <= FUSION_FIT_TRIALS))
    tgt = case["es"][:, None] == case["ts"][None, :]
    if tgt.shape != (m, nt):                                         # (the width changed: labels of the new width)
        case["es"], case["ts"] = trials_labels(rng, m, nt, pick.hits["layout"])
        tgt = case["es"][:, None] == case["ts"][None, :]
    # K systems on one trial set, each of the drawn content in its own units, with its own pitch and base offset
    if form == "pass":
        S = [(np.float32(FUSION_UNITS[j]) * trials_scores(rng, m, nt, nt, tgt, case["content"]) - np.float32(0.5 * j)).astype(np.float32)
             for j in range(k)]
    else:                                        # correlated systems (a common part plus own noise), or K of them are separable
        base = trials_scores(rng, m, nt, nt, tgt, "inverted" if case["content"] == "inverted" else "gaussian").astype(np.float64)
        S = [FUSION_UNITS[j] * (base + 1.5 * rng.standard_normal((m, nt))) - 0.5 * j for j in range(k)]
        if case["content"] in ("ties8", "zeros_mix"):
            S = [np.round(s) for s in S]
        S = [s.astype(np.float32) for s in S]
        if case["content"] == "zeros_mix":
            for s_ in S:
                z = s_ == 0
                s_[z] = np.where(rng.random(int(z.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    ld_kinds = [pick.hits["ld"]] + [str(rng.choice(TRIALS_MENUS["ld"])) for _ in range(k - 1)]
    case.update(k=k, systems=S, lds=[trials_ld(kind, nt) for kind in ld_kinds], offs=[case["off"]] + [int(rng.integers(0, 2)) for _ in range(k - 1)])
    del case["S"], case["ld"], case["off"]
    if form == "pass":
        kind = pick("point", rank)
        a, c = {"start": (np.zeros(k), 0.0), "alone": (np.eye(k)[k - 1], -0.25),
                "cancel": (np.array([(-1.0) ** j / FUSION_UNITS[j] for j in range(k)]), 0.125),
                "drawn": (rng.uniform(-1.0, 1.0, k) / np.asarray(FUSION_UNITS[:k]), float(rng.uniform(-3.0, 3.0)))}[kind]
        case["a"], case["c"] = np.asarray(a, np.float64), float(c)
        # (the rule's band holds where (K + 1) Ymax <= 2000: these points keep |y| below a few dozen)
        assert (k + 1) * (abs(c) + sum(abs(x) * float(np.abs(s).max()) for x, s in zip(a, S))) <= 2000.0
        what += " " + _opts(K=k, point=kind)
    else:
        prior = pick("prior", rank)
        pos, neg = fm.split(S, case["es"], case["ts"])
        try:
            f = fm.fit(pos, neg, prior)
        except ValueError as e:
            raise IllPosed(str(e))
        if not f["converged"] or f["separable"]:
            raise IllPosed("converged %s separable %s" % (f["converged"], f["separable"]))
        case["prior"] = prior
        what += " " + _opts(K=k, prior=prior)
    case.update(form=form, what="%dx%d %s form=%s" % (m, nt, what.split(" ", 1)[1], form))
    return case


_GENERATORS["fusion"] = _draw_fusion


# ------------------------------------------------------------------------------------------- transform (K4, csrc/transform.hip)
# Dout: the edges of the five dimension classes of the one-pass kernel and one past each (513: the GEMM + length-norm pair); Din =
# Dout + ragged (not a multiple of the 4-wide k-step or of the 16-deep stage); the row counts are written in the plan's own
# terms -- G compute units, R0 rows of a main block (plda_transform_plan) -- and resolved on the device by transform_rows().
MENUS["transform"] = {
    "dout": (1, 17, 127, 128, 129, 208, 209, 256, 257, 384, 385, 512, 513),
    "ragged": (0, 1, 3, 5),
    "rows": ("1", "17", "16G", "16G+1", "32G+1", "64G+1", "R0G", "R0G+1", "R0G+16G+1"),
    "form": ("uniform", "perrow"),
    "arm": ("fused", "fused", "pair"),               # pair: PLDA_TRANSFORM_VARIANT=1 (and whatever Dout > 512 takes)
    "mean": (0.0, 1.0, 1e3),                         # |mean| in spreads of the rows
    "uniform": (1, 3, 4096),
}


def transform_rows(entry, g, r0):
    """the row count of a "rows" entry on a device of g compute units whose class has main blocks of r0 rows"""
    return {"1": 1, "17": 17, "16G": 16 * g, "16G+1": 16 * g + 1, "32G+1": 32 * g + 1, "64G+1": 64 * g + 1, "R0G": r0 * g,
            "R0G+1": r0 * g + 1, "R0G+16G+1": r0 * g + 16 * g + 1}[entry]


def transform_shapes(entry, r0):
    """the launches a "rows" entry takes on the one-pass arm, as transform_model.shapes_of reports them (the same on any CU count)"""
    tail64 = ("tail", 64)                            # (for r0 = 64 that is the main shape used as a tail)
    return {"1": {("tail", 16)}, "17": {("tail", 16)}, "16G": {("tail", 16)}, "16G+1": {("tail", 32)}, "32G+1": {tail64},
            "64G+1": {("tail", 128)} if r0 == 128 else {("main", 64), ("tail", 16)}, "R0G": {("main", r0)},
            "R0G+1": {("main", r0), ("tail", 16)}, "R0G+16G+1": {("main", r0), ("tail", 32)}}[entry]


def _draw_transform(pick, rng):
    import transform_model as M
    dout, ragged, rows, (form, frank) = pick("dout"), pick("ragged"), pick("rows"), pick.cycle("form")
    (arm, _), mean_size = pick.cycle("arm"), pick("mean")
    if dout > 512:
        arm = pick.force("arm", "pair")
    din = dout + ragged
    model = M.make_model(rng, din, dout, mean_size)
    x, n = M.pool_rows(rng, din, model[0])
    uniform = pick("uniform", frank) if form == "uniform" else None
    case = dict(din=din, dout=dout, rows=rows, form=form, arm=arm, model=model, x=x, n=n, uniform=uniform,
                index_seed=int(rng.integers(1 << 30)))
    case["what"] = "%dx%d " % (din, dout) + _opts(rows=rows, form=form, arm=arm, mean=mean_size, uniform=uniform)
    return case


_GENERATORS["transform"] = _draw_transform
