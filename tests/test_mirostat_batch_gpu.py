"""GPU: Mirostat members in k_sample_batch.  An 8-slot table holds three Mirostat samplers (different tau, eta and seed, one of them in the
fallback regime), two chain samplers, one greedy member through the sampler, one sampler at a forced position and one empty slot; over 16
launches every bound slot leaves what its twin, driven alone by bitnet_hip_sample_dev, leaves: tokens, histories, positions, mu bits, fallback
counts and word counters, bit for bit (one kernel body serves both entry points)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

VOCAB, N_SLOTS, HIST, LAUNCHES = 4099, 8, 32, 16
# (config, chain keywords, Mirostat (tau, eta) or None, forced positions)
MEMBERS = [((0.7, 0, 1.0, 1.1), dict(frequency_penalty=0.2, presence_penalty=0.1), (5.0, 0.1), 0),
           ((1.0, 0, 1.0, 1.0), {}, (8.0, 0.25), 0),
           ((1.0, 0, 1.0, 1.0), {}, (0.5, 0.1), 0),                                # the fallback on every call
           ((0.8, 0, 0.95, 1.1), dict(min_p=0.05, typical_p=0.9), None, 0),        # chain, full-vocabulary path
           ((0.8, 40, 0.95, 1.1), dict(min_p=0.05), None, 0),                      # chain, one-lane path
           ((0.0, 0, 1.0, 1.1), {}, None, 0),                                      # greedy through the sampler
           ((0.7, 0, 1.0, 1.0), {}, (5.0, 0.1), HIST)]                             # Mirostat at a forced position: every step of the run


def test_batch_slots_equal_sample_dev_alone(hip):
    import torch

    rng = np.random.default_rng(123)

    def lane(i):
        cfg, ex, miro, forced = MEMBERS[i]
        smp = hip.sampler(VOCAB, *cfg, seed=700 + i, **ex)
        if miro:
            smp.set_mirostat(*miro)
        hist = torch.full((HIST,), -1, dtype=torch.int32, device="cuda")
        if forced:
            hist.copy_(torch.arange(100, 100 + HIST, dtype=torch.int32))
        return dict(smp=smp, tok=torch.full((1,), -1, dtype=torch.int32, device="cuda"), pos=torch.zeros(1, dtype=torch.int32, device="cuda"),
                    hist=hist, nf=torch.full((1,), forced, dtype=torch.int32, device="cuda"),
                    logits=torch.zeros(VOCAB, dtype=torch.float32, device="cuda"))

    members, twins = [lane(i) for i in range(len(MEMBERS))], [lane(i) for i in range(len(MEMBERS))]
    table = hip.sample_batch(VOCAB, N_SLOTS)
    slots = [0, 1, 2, 3, 4, 5, 7]  # slot 6 stays empty
    for b, m in zip(slots, members):
        table.set(b, m["smp"], m["logits"], m["tok"], m["pos"], m["hist"], m["nf"])
    for call in range(LAUNCHES):
        for m, t in zip(members, twins):
            x = torch.from_numpy((2.0 * rng.standard_normal(VOCAB)).astype(np.float32))
            m["logits"].copy_(x)
            t["logits"].copy_(x)
        table.launch()
        for t in twins:
            t["smp"].sample_dev(t["logits"], t["tok"], t["pos"], t["hist"], t["nf"])
        torch.cuda.synchronize()
        for i, (m, t) in enumerate(zip(members, twins)):
            for key in ("tok", "pos", "hist"):
                assert torch.equal(m[key], t[key]), (call, i, key, m[key], t[key])
            sm, st = m["smp"].mirostat_state(), t["smp"].mirostat_state()
            assert np.float32(sm[0]).tobytes() == np.float32(st[0]).tobytes() and sm[1] == st[1], (call, i, sm, st)
            assert m["smp"].draws() == t["smp"].draws(), (call, i)
            assert int(m["pos"].item()) == call + 1
    mu = [m["smp"].mirostat_state() for m in members]
    draws = [m["smp"].draws() for m in members]
    assert mu[0][0] != 10.0 and mu[1][0] != 16.0 and draws[0] + mu[0][1] == LAUNCHES and draws[1] + mu[1][1] == LAUNCHES
    assert mu[2][1] == LAUNCHES and draws[2] == 0 and mu[2][0] < 1.0       # the fallback regime: no word, mu moving down
    assert mu[3] == mu[4] == mu[5] == (0.0, 0) and draws[3] == draws[4] == LAUNCHES and draws[5] == 0
    assert mu[6] == (10.0, 0) and draws[6] == 0                            # forced: nothing moved, mu included
    assert members[6]["tok"].item() == 100 + LAUNCHES
    # the hand-over was re-armed: one more call alone on either side gives the same token and state
    for b, m, t in zip(slots, members, twins):
        table.set(b, None)
        for l in (m, t):
            l["smp"].sample_dev(l["logits"], l["tok"], l["pos"], l["hist"], l["nf"])
        torch.cuda.synchronize()
        assert torch.equal(m["tok"], t["tok"]) and torch.equal(m["hist"], t["hist"]) and m["smp"].mirostat_state() == t["smp"].mirostat_state()
    table.close()
    for l in members + twins:
        l["smp"].close()
