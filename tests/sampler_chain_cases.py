"""Case lists of the sampler chain (min-p, typical-p, frequency / presence penalty) as module-level data -- test infrastructure.
tests/test_sampler_chain_gpu.py runs them on the device; tests/test_sampler_chain_accept.py walks the same lists on the CPU.

A case is a case of tests/sampler_cases.py (rows and generated lists come from there) with one more key, ex = dict(min_p, typical_p,
frequency_penalty, presence_penalty).  Rows are sigma = 4 normal rows throughout; sigma = 2 rows appear only behind min_p >= 0.02 (flat rows
put thousands of near-equal deviations around the typical-p cut), and at vocabulary 128256 typical_p stays <= 0.5 unless min-p runs in front."""
from __future__ import annotations

import sampler_cases as sc

NEUTRAL = dict(min_p=0.0, typical_p=1.0, frequency_penalty=0.0, presence_penalty=0.0)


def _case(cid, vocab, cfg, seed, row_, steps=1, gen_=(), **ex):
    return dict(sc._case(cid, vocab, cfg, seed, row_, gen_, steps), ex=dict(NEUTRAL, **ex))


# ---- path G: the additive penalties in front of the argmax --------------------------------------------------------------------------
# two_top: ids 0 and 1 hold 10 and 9, so the favourite changes as the counts grow (and the occurrence count parts from the compounding
# exponent at the third call); pen: the penalised ids 0..4 hold +x, -x, +0.0, -0.0 and -inf
G_EX = dict(frequency_penalty=0.5, presence_penalty=0.3)
GREEDY = [_case(f"chain-G-v{v}-{r[0]}", v, (0.0, 0, 1.0, 1.1), 7000, r, 8, g, **G_EX)
          for v in (1000, 128256) for r, g in ((("two_top",), ()), (("pen", 2.0), (0, 1, 2, 3, 4, 0, 0)))]
GREEDY += [_case("chain-G-v1000-bonus", 1000, (1.0, 0, 1.0, 1.0), 7001, ("two_top",), 4, (), frequency_penalty=-0.25, presence_penalty=0.0)]

# ---- path S: the stages over the k survivors in one lane ----------------------------------------------------------------------------
S_CONFIGS = [("minp", dict(min_p=0.05)), ("typ", dict(typical_p=0.9)), ("both", dict(min_p=0.05, typical_p=0.9)),
             ("typ0", dict(typical_p=0.0)), ("all", dict(min_p=0.1, typical_p=0.5, frequency_penalty=0.2, presence_penalty=0.1))]
SMALL = [_case(f"chain-S-v{v}-{name}-s{si}", v, (0.8, 40, 0.95, 1.1), 7100 + 13 * ci + si, ("normal", 4.0), 3, (), **ex)
         for v in (1000, 128256) for ci, (name, ex) in enumerate(S_CONFIGS) for si in range(3 if v == 1000 else 1)]
# exact rows: every sum is exact, so `>=` against `>`, the cut off by one and the order of tied deviations all show
SMALL += [_case(f"chain-S-v1000-equal-typ-s{si}", 1000, (0.8, 64, 1.0, 1.0), 7200 + si, ("equal",), 1, (), typical_p=0.5) for si in range(8)]
SMALL += [_case(f"chain-S-v1000-interleaved-minp1-s{si}", 1000, (0.8, 64, 1.0, 1.0), 7220 + si, ("two_interleaved",), 1, (), min_p=1.0) for si in range(4)]
SMALL += [_case(f"chain-S-v1000-{r[0]}-both", 1000, (0.8, 40, 0.9, 1.0), 7240 + ri, r, 1, (), min_p=0.05, typical_p=0.9)
          for ri, r in enumerate([("all_neginf",), ("one_inf",), ("neginf_but_one",), ("planted", 4.0)])]

# ---- path F: min-p as one more cut of the descending order ---------------------------------------------------------------------------
F_VOCABS = [1025, 2049, 32000, 128256]
F_CONFIGS = [("minp", (0.8, 0, 1.0, 1.0), dict(min_p=0.05)),
             ("topp-minp", (0.8, 0, 0.9, 1.1), dict(min_p=0.05)),
             ("k65-minp", (1.0, 65, 1.0, 1.0), dict(min_p=0.1)),
             ("minp-pen", (0.9, 0, 1.0, 1.1), dict(min_p=0.02, frequency_penalty=0.2, presence_penalty=0.1))]
FULL = [_case(f"chain-F-v{v}-{name}-sig{sig:g}", v, cfg, 7300 + 7 * ci + (v % 97), ("normal", sig), 6, (), **ex)
        for v in F_VOCABS for ci, (name, cfg, ex) in enumerate(F_CONFIGS) for sig in (4.0, 2.0)]
MINP_ONLY = [c for c in FULL if c["ex"]["typical_p"] >= 1]

# ---- path F: typical-p, a second selection over the deviations ------------------------------------------------------------------------
def _typ_configs(v):
    alone = 0.9 if v < 128256 else 0.5
    return [("typ", (0.8, 0, 1.0, 1.0), dict(typical_p=alone), (4.0,)),
            ("topp-minp-typ", (0.8, 0, 0.9, 1.1), dict(min_p=0.05, typical_p=0.9), (4.0, 2.0)),
            ("k65-typ", (1.0, 65, 1.0, 1.0), dict(typical_p=0.5), (4.0,)),
            ("minp-typ-pen", (0.9, 0, 1.0, 1.1), dict(min_p=0.02, typical_p=0.2, frequency_penalty=0.2, presence_penalty=0.1), (4.0, 2.0))]


FULL_TYP = [_case(f"chain-F-v{v}-{name}-sig{sig:g}", v, cfg, 7500 + 7 * ci + (v % 97), ("normal", sig), 6, (), **ex)
            for v in F_VOCABS for ci, (name, cfg, ex, sigs) in enumerate(_typ_configs(v)) for sig in sigs]

# ---- exact rows on path F ------------------------------------------------------------------------------------------------------------
EXACT_F = [_case(f"chain-F-v2049-equal_one-{w}-s{si}", 2049, (1.0, 0, 1.0, 1.0), 7400 + si, ("equal_one", w), 1, (), min_p=0.5)
           for w in ("slice-1", "slice", "last") for si in range(2)]
EXACT_F += [_case(f"chain-F-v1025-interleaved-minp1-s{si}", 1025, (0.7, 0, 1.0, 1.0), 7420 + si, ("two_interleaved",), 1, (), min_p=1.0) for si in range(8)]
EXACT_F += [_case(f"chain-F-v1025-{r[0]}-minp", 1025, (0.7, 0, 0.9, 1.0), 7440 + ri, r, 1, (), min_p=0.05)
            for ri, r in enumerate([("all_neginf",), ("one_inf",), ("neginf_but_one",), ("planted", 4.0)])]

# all deviations tie and every sum is exact: typical_p 0.5 of 64 equal entries keeps ids 0..31 (`>=`, ascending id); vocab 64 with top_k 0 is path F
EXACT_F += [_case(f"chain-F-v64-equal-typ-s{si}", 64, (0.8, 0, 1.0, 1.0), 7460 + si, ("equal",), 1, (), typical_p=0.5) for si in range(8)]
EXACT_F += [_case(f"chain-F-v2049-equal-typ-s{si}", 2049, (0.8, 0, 1.0, 1.0), 7470 + si, ("equal",), 1, (), typical_p=0.25) for si in range(2)]
EXACT_F += [_case(f"chain-F-v1025-{r[0]}-typ", 1025, (0.7, 0, 0.9, 1.0), 7480 + ri, r, 1, (), min_p=0.05, typical_p=0.9)
            for ri, r in enumerate([("all_neginf",), ("one_inf",), ("neginf_but_one",), ("planted", 4.0)])]

ALL = GREEDY + SMALL + FULL + FULL_TYP + EXACT_F
assert len({c["id"] for c in ALL}) == len(ALL)
