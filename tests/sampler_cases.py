"""The sampler case lists as module-level data -- test infrastructure.  test_sampling_gpu.py runs them on the device;
test_sampler_accept.py walks exactly the same lists on the CPU (the reference's token, an exact float64 sampler and its mutants
through `sampler_accept.accepts`).

A case is a dict: id, vocab, cfg = (temperature, top_k, top_p, repetition_penalty), seed, row = (family, *args), gen = the
generated list handed to the first call (`sample_host`), steps = calls in a row on one sampler, each fed the growing list of the
tokens chosen so far (what `sample_dev` counts by itself).  `row(case)` and `gen(case)` materialise the data, deterministically
from the case alone."""
from __future__ import annotations

import zlib

import numpy as np

SMALL_K = 64
MAX_VOCAB = 1 << 20


def geometry(vocab: int) -> tuple[int, int]:
    """(workgroups, slice) of the launch: csrc/kernels_sample.hip bitnet_hip_sampler_create."""
    nwg = min(64, -(-vocab // 1024))
    return nwg, -(-vocab // nwg)


def _rng(case, salt=0):
    return np.random.default_rng(zlib.crc32(case["id"].encode()) + salt)


def _kth(x, k):
    """the k-th largest value (k >= 1)"""
    return np.partition(x, x.size - k)[x.size - k]


def row(case) -> np.ndarray:
    fam, *args = case["row"]
    v = case["vocab"]
    k = case["cfg"][1]
    rng = _rng(case)
    nwg, sl = geometry(v)
    if fam == "normal":
        x = (args[0] * rng.standard_normal(v)).astype(np.float32)
    elif fam == "equal":
        x = np.full(v, 0.5, np.float32)
    elif fam == "equal_one":  # every entry equal but a single larger one
        x = np.full(v, 0.5, np.float32)
        x[{"first": 0, "slice-1": sl - 1, "slice": min(sl, v - 1), "last": v - 1}[args[0]]] = 3.0
    elif fam == "two_interleaved":
        x = np.where(np.arange(v) % 2 == 0, 1.0, 0.0).astype(np.float32)
    elif fam == "two_blocks":
        x = np.where(np.arange(v) < v // 2, 0.0, 1.0).astype(np.float32)
    elif fam == "kth_dup":  # the k-th value 200 times, straddling every workgroup slice boundary
        x = rng.standard_normal(v).astype(np.float32)
        kth = _kth(x, k if 0 < k < v else 100)
        pos = [b + d for b in range(sl, v, sl) for d in (-1, 0, 1) if b + d < v][:200]
        free = np.setdiff1d(np.arange(v), pos)
        pos += [int(i) for i in rng.choice(free, 200 - len(pos), replace=False)]
        x[pos] = kth
    elif fam == "zeros":
        x = np.where(rng.integers(0, 2, v) == 0, 0.0, -0.0).astype(np.float32)
    elif fam in ("one_inf", "two_inf"):
        x = rng.standard_normal(v).astype(np.float32)
        x[rng.choice(v, 1 if fam == "one_inf" else 2, replace=False)] = np.inf
    elif fam == "neginf_but_one":
        x = np.full(v, -np.inf, np.float32)
        x[int(rng.integers(0, v))] = 1.5
    elif fam == "all_neginf":
        x = np.full(v, -np.inf, np.float32)
    elif fam == "huge":  # +-3e38: overflows to +-inf once divided by a temperature below 1
        x = np.where(rng.integers(0, 2, v) == 0, 3e38, -3e38).astype(np.float32)
    elif fam == "subnormal":
        x = (rng.integers(1, 1 << 23, v).astype(np.uint32) | (rng.integers(0, 2, v).astype(np.uint32) << 31)).view(np.float32).copy()
    elif fam == "planted":  # a normal row with NaN, -inf, +-0 and duplicates planted (the existing grid's kind)
        x = (args[0] * rng.standard_normal(v)).astype(np.float32)
        if v >= 16:
            idx = rng.choice(v, 8, replace=False)
            x[idx[0]], x[idx[1]], x[idx[2]], x[idx[3]] = np.nan, -np.inf, 0.0, -0.0
            x[idx[4:6]] = x[idx[6]]
    elif fam == "two_top":  # two close favourites: the compounded exponent tips the first below the second at the third call
        x = rng.standard_normal(v).astype(np.float32)
        x[:2] = [10.0, 9.0]
    elif fam == "pen":  # penalty edges: the penalised ids 0..4 hold +x, -x, +0.0, -0.0, -inf
        x = rng.standard_normal(v).astype(np.float32)
        x[:5] = [args[0], -args[0], 0.0, -0.0, -np.inf]
    else:
        raise ValueError(fam)
    return x


def gen(case) -> list[int]:
    g = case.get("gen", ())
    if g and g[0] == "rand":  # ("rand", n, distinct): n tokens drawn from `distinct` ids
        rng = _rng(case, 1)
        ids = rng.choice(case["vocab"], min(g[2], case["vocab"]), replace=False)
        return [int(t) for t in rng.choice(ids, g[1])]
    return [int(t) for t in g]


def _case(cid, vocab, cfg, seed, row_, gen_=(), steps=1):
    return dict(id=cid, vocab=vocab, cfg=cfg, seed=seed, row=row_, gen=gen_, steps=steps)


# ---- the vocabulary sweep ----------------------------------------------------------------------------------------------------
SWEEP_VOCABS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 32000, 50257, 65536, 65537, 128256, 151936, MAX_VOCAB - 1, MAX_VOCAB]


def sweep_configs(v):
    """(label, cfg) that make sense at vocabulary v; duplicates dropped."""
    out = [("G", (1.0, 0, 1.0, 1.1))]
    if v > 1:
        out.append(("S", (0.8, min(64, v - 1), 0.9, 1.1)))
    f = [(0.7, 0, 0.9, 1.1), (1.0, 65, 1.0, 1.0), (1.3, v - 1, 0.95, 1.0), (0.7, v, 1.0, 1.1), (1.3, v + 7, 0.5, 1.0), (0.9, 0, 0.999999, 1.0),
         (1.0, 0, 1e-6, 1.0)]
    seen = set()
    for cfg in f:
        small = 0 < cfg[1] <= SMALL_K and cfg[1] < v
        if small or cfg in seen:
            continue  # lands on the S path at this size
        seen.add(cfg)
        out.append(("F", cfg))
    return out


def _sweep():
    # two calls per case (the second sees a penalised token), one at the two largest sizes to keep the CPU walk short
    cases = []
    for v in SWEEP_VOCABS:
        for ci, (label, cfg) in enumerate(sweep_configs(v)):
            sigma = (1.0, 4.0, 12.0)[ci % 3]
            g = ("rand", 9, 4) if cfg[3] != 1.0 else ()
            cases.append(_case(f"sweep-v{v}-{label}{ci}", v, cfg, 3000 + 31 * ci + v % 977, ("planted", sigma), g, steps=2 if v < 200000 else 1))
    return cases


SWEEP = _sweep()

# ---- adversarial rows --------------------------------------------------------------------------------------------------------
ADV_VOCABS = [1025, 65537, 128256]
ADV_ROWS = [("equal",), ("equal_one", "first"), ("equal_one", "slice-1"), ("equal_one", "slice"), ("equal_one", "last"), ("two_interleaved",),
            ("two_blocks",), ("normal", 0.05), ("kth_dup",), ("zeros",), ("one_inf",), ("two_inf",), ("neginf_but_one",), ("all_neginf",),
            ("subnormal",)]


def adv_configs(v):
    return [("S", (0.8, 40, 0.9, 1.0)), ("F", (1.3, 0, 0.5, 1.0)), ("F", (1.0, 65, 1.0, 1.0)), ("F", (0.7, v // 2, 0.95, 1.0))]


def _adversarial():
    cases = []
    for v in ADV_VOCABS:
        for ri, r in enumerate(ADV_ROWS):
            for ci, (label, cfg) in enumerate(adv_configs(v)):
                cases.append(_case(f"adv-v{v}-{'-'.join(str(a) for a in r)}-{label}{ci}", v, cfg, 5000 + 17 * ri + ci, r))
        for ci, (label, cfg) in enumerate([("S", (0.5, 40, 0.9, 1.0)), ("F", (0.5, 0, 0.9, 1.0)), ("F", (0.5, 65, 1.0, 1.0))]):
            cases.append(_case(f"adv-v{v}-huge-{label}{ci}", v, cfg, 5400 + ci, ("huge",)))
        for t in (1e-30, 1e30):  # 1e-30 overflows every entry; 1e30 flattens the row (and a subnormal row to +-0)
            for ci, (label, k, p) in enumerate([("S", 40, 0.9), ("F", 0, 0.9), ("F", 65, 1.0)]):
                cases.append(_case(f"adv-v{v}-t{t:g}-normal-{label}{ci}", v, (t, k, p, 1.0), 5500 + ci, ("normal", 1.0)))
                cases.append(_case(f"adv-v{v}-t{t:g}-subnormal-{label}{ci}", v, (t, k, p, 1.0), 5600 + ci, ("subnormal",)))
    # a float64 sum that equals top_p exactly: an all-equal row of 2^j entries (every sum is exact in f32 too), top_p 0.5.  The
    # reference keeps entries while cumsum <= top_p, so it keeps vocab / 2 + 1 of them
    for v in (2, 64, 2048):
        for si in range(3):
            cases.append(_case(f"adv-v{v}-equal-topp-tie-F{si}", v, (0.7, 0, 0.5, 1.0), 5700 + si, ("equal",)))
    return cases


ADVERSARIAL = _adversarial()

# ---- penalty edges -----------------------------------------------------------------------------------------------------------
# ids 0..4 hold +x, -x, +0.0, -0.0, -inf and are repeated until powi(rp, count) reaches inf (rp 2, 1e10) or 0 (rp 0.5): 200
# repeats give 2^200 -> inf and 0.5^200 -> 0 in f32, so x / inf, x * inf, 0 * inf (NaN -> -inf) and x / 0 all occur.  A few
# repeats (3) keep the power finite.
def _penalty():
    cases = []
    for v in (1025, 128256):
        for rp in (0.5, 2.0, 1e10):
            for reps in (3, 200):
                g = tuple([0, 1, 2, 3, 4] * reps)
                for ci, (label, cfg) in enumerate([("G", (1.0, 0, 1.0, rp)), ("S", (0.8, 40, 0.9, rp)), ("F", (0.7, 0, 1.0, rp)), ("F", (1.3, 0, 0.9, rp)),
                                                   ("F", (1.0, 65, 1.0, rp))]):
                    for x0 in (2.0, 40.0):
                        cases.append(_case(f"pen-v{v}-rp{rp:g}-reps{reps}-x{x0:g}-{label}{ci}", v, cfg, 6000 + ci, ("pen", x0), g))
    # a long list: 4096 tokens from 50 distinct ids, through sample_host
    for ci, (label, cfg) in enumerate([("G", (1.0, 0, 1.0, 1.1)), ("S", (0.8, 40, 0.9, 1.3)), ("F", (0.7, 0, 0.9, 1.1)), ("F", (1.0, 65, 1.0, 1.02))]):
        cases.append(_case(f"pen-long-{label}{ci}", 128256, cfg, 6100 + ci, ("normal", 4.0), ("rand", 4096, 50)))
    # multi-call sequences: the exponent compounds (count_exponent), which a single call cannot show
    for v in (1025, 128256):
        for ci, (label, cfg) in enumerate([("G", (1.0, 0, 1.0, 1.5)), ("S", (0.8, 40, 0.9, 1.5)), ("F", (0.7, 0, 0.9, 1.5)), ("F", (1.0, 65, 1.0, 1.5))]):
            cases.append(_case(f"pen-seq-v{v}-{label}{ci}", v, cfg, 6200 + ci, ("normal", 12.0), (), steps=6))
        cases.append(_case(f"pen-seq-v{v}-two_top-G", v, (1.0, 0, 1.0, 1.05), 6300, ("two_top",), (), steps=4))
    return cases


PENALTY = _penalty()

# ---- the ends of the draw ------------------------------------------------------------------------------------------------------
# Seeds found by scanning ChaCha20Rng(seed).random_f32() on the CPU (test_sampler_accept.py asserts the property of each u):
SEED_U_LOW = 294583    # first u < 2^-16
SEED_U_HIGH = 62435    # first u >= 1 - 2^-16
SEED_U_PAST_TOTAL = 62435  # first u above the f32 total of the flat 128256-entry row at temperature 0.7 (asserted too)
ENDS_VOCAB = 128256


def _ends():
    cases = []
    for name, seed in (("low", SEED_U_LOW), ("high", SEED_U_HIGH)):
        for r in (("equal",), ("normal", 4.0)):
            for ci, cfg in enumerate([(0.7, 0, 0.9, 1.0), (1.3, 0, 0.999999, 1.0), (1.0, 65, 1.0, 1.0), (0.7, 5000, 1.0, 1.0)]):
                cases.append(_case(f"ends-{name}-{r[0]}-F{ci}", ENDS_VOCAB, cfg, seed, r))
    # the reference's fall-through: u beyond an f32 total that ended below 1 (no top-p, so the sums run over the whole row)
    cases.append(_case("ends-past-total-two_blocks", ENDS_VOCAB, PAST_TOTAL_CFG, SEED_U_PAST_TOTAL, PAST_TOTAL_ROW))
    return cases


PAST_TOTAL_CFG = (0.7, 0, 1.0, 1.0)
PAST_TOTAL_ROW = ("two_blocks",)
ENDS = _ends()

ALL = SWEEP + ADVERSARIAL + PENALTY + ENDS
assert len({c["id"] for c in ALL}) == len(ALL)
