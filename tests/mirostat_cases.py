"""Seeded inputs of the Mirostat tests -- test infrastructure.  tests/test_mirostat_ref.py walks them on the CPU (the restatement, a numpy model
of the kernel's arithmetic, the loose-draw cap), tests/test_mirostat_gpu.py runs them on the device.

A case: id, vocab, sigma (the row is N(0, sigma^2), drawn once from `seed`), tau, eta, temperature, and the penalties (repetition, frequency,
presence; 1 / 0 / 0: off).  Every case is 32 chained calls on its row; with penalties on, the counts accumulate over them.
Regimes (tau, sigma): (5, 2) keeps a few hundred entries, the threshold in the tail; (8, 1) keeps nearly everything; (0.5, 1) falls back on
every call and mu runs negative; (3, 1) at vocab >= 32000 falls back on every call."""
from __future__ import annotations

import numpy as np

STEPS = 32
LOOSE_CAP = 1 / 8  # of a case's draws

PEN_ON = dict(repetition_penalty=1.1, frequency_penalty=0.2, presence_penalty=0.1)
PEN_OFF = dict(repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0)


def _case(vocab, tau, sigma, temperature, pen, seed, eta=0.1):
    name = f"v{vocab}-tau{tau}-s{sigma}-T{temperature}-{'pen' if pen is PEN_ON else 'plain'}"
    return dict(id=name, vocab=vocab, tau=tau, eta=eta, sigma=sigma, temperature=temperature, seed=seed, steps=STEPS, **pen)


def _build():
    out, k = [], 0
    for vocab in (1, 2, 257, 1025, 4099):
        for tau, sigma in ((5.0, 2.0), (8.0, 1.0), (0.5, 1.0)):
            out.append(_case(vocab, tau, sigma, (0.7, 1.0)[k % 2], (PEN_ON, PEN_OFF)[(k // 2) % 2], 1000 + k))
            k += 1
    # every temperature x penalty combination in the regime where the threshold cuts the tail, slices of unequal length
    for temperature in (0.7, 1.0):
        for pen in (PEN_ON, PEN_OFF):
            out.append(_case(4099, 5.0, 2.0, temperature, pen, 2000 + k))
            k += 1
    out.append(_case(32003, 3.0, 1.0, 1.0, PEN_OFF, 3000))   # the fallback on every call at a large vocabulary
    # the flagship vocabulary, once.  sigma 4: at sigma 2 the reference's own sequential f32 sum drifts by 1.6e-4 in ln S over 128256 terms,
    # the band follows it, and 7 of 32 draws were loose (tests/test_mirostat_ref.py holds the cap for the restatement alone)
    out.append(_case(128256, 5.0, 4.0, 0.7, PEN_ON, 3003))
    ids = [c["id"] for c in out]
    dup = {i for i in ids if ids.count(i) > 1}
    for c in out:
        if c["id"] in dup:
            c["id"] += f"-seed{c['seed']}"
    return out


CASES = _build()


def row(case) -> np.ndarray:
    return (case["sigma"] * np.random.default_rng(case["seed"]).standard_normal(case["vocab"])).astype(np.float32)


def ref_kwargs(case) -> dict:
    return dict(tau=case["tau"], eta=case["eta"], seed=case["seed"], temperature=case["temperature"], repetition_penalty=case["repetition_penalty"],
                frequency_penalty=case["frequency_penalty"], presence_penalty=case["presence_penalty"])


# ---- edge rows: (name, row, temperature) ------------------------------------------------------------------------------------------------
def edge_rows(vocab: int = 2500):
    base = np.random.default_rng(77).standard_normal(vocab).astype(np.float32)
    ninf, nan = np.float32(-np.inf), np.float32(np.nan)
    one_inf = base.copy()
    one_inf[[7, vocab - 300]] = np.inf  # two of them, in different workgroup slices: the fallback takes the last
    single = np.full(vocab, ninf, np.float32)
    single[1234] = 2.5
    return [("all-neg-inf", np.full(vocab, ninf, np.float32), 1.0), ("all-nan", np.full(vocab, nan, np.float32), 1.0), ("pos-inf", one_inf, 1.0),
            ("single-finite", single, 1.0), ("temperature-overflow", (30.0 * base).astype(np.float32), 1e-37)]


def tie_row(vocab: int, where: list[int], seed: int = 5) -> np.ndarray:
    """N(0, 1) with one duplicated maximum at the ids `where`"""
    x = np.random.default_rng(seed).standard_normal(vocab).astype(np.float32)
    x[where] = np.float32(6.0)
    return x
