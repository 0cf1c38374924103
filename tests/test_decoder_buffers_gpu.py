"""The host decoders' device memory (host/dev_buffer.hpp) on the GPU, on model A of tests/test_decoder_state_gpu.py (QK256, f32 cache).

(a) life cycle  an owner, a borrower and a 2-slot batch drive every site that grows a buffer once; after batch, borrower and owner are
                released -- and again with the owner's handle released FIRST, the borrower keeping it alive -- bitnet_host_device_bytes()
                is back where it started: every allocation freed, none of the borrowed ones twice (a double hipFree is an error the
                runtime reports, and the counter would fall below its start).  The f16 activation chain's buffers grow in a child
                process, under BITNET_HOST_PREFILL_CHAIN=1.
(b) growth      prefill, score and step_wide: a small call, a larger one, a reset and the small call again leave the SHA-256 of
                last_logits, last_hidden and the layer-0 K and V caches of a fresh decoder that made only the last call -- the cache slots
                below the position, which are the sequence's: reset() leaves the cache bytes, so the slots beyond still hold the larger
                call's rows, as they always have --; and the counter after the larger call is that of a fresh decoder that made only the
                larger call -- growth frees the old group.
(c) position 0  set_logprobs, then reset, on a decoder at position 0: logprobs() reads cleared records."""
import hashlib
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_read as kv  # noqa: E402
from test_decoder_state_gpu import MODELS  # noqa: E402

pytestmark = pytest.mark.gpu


class Model:
    def __init__(self, pkg):
        synth = importlib.import_module("bitnet-rs_amd.synth")
        self.pkg = pkg
        self.cfg = synth.ModelConfig(**MODELS["A"])
        self.glob = synth.make_globals(self.cfg)
        self.layers = [synth.make_layer(self.cfg, l) for l in range(self.cfg.n_layers)]
        self.toks = synth.prompt(self.cfg.max_pos, self.cfg.vocab)

    def decoder(self):
        dec = self.pkg.HostDecoder(self.cfg)
        for l, w in enumerate(self.layers):
            dec.set_layer_qk256(l, w)
        dec.set_globals(self.glob)
        dec.reset()
        return dec

    def fresh(self, dec, n_fed):
        dec.reset()
        dec.feed(self.toks[:n_fed])


@pytest.fixture(scope="module")
def model(pkg, hip):
    return Model(pkg)


def drive_every_growth_site(M, owner, bor, batch):
    """-> the counter's largest value on the way"""
    peak = 0

    def seen():
        nonlocal peak
        peak = max(peak, M.pkg.host_device_bytes())

    M.fresh(owner, 21)
    owner.prefill(21, with_logits=True, digits=2)       # ensure_prompt_buffers, the f16 hand-over rows
    seen()
    M.fresh(owner, 131)
    owner.prefill(130, with_logits=True, digits=2)      # ... grown
    seen()
    owner.extend(1, with_logits=True, digits=2)
    M.fresh(owner, 40)
    owner.score(40, digits=2, logits_rows=0)            # the sc_* group
    owner.reset()
    owner.feed(M.toks[:50])
    owner.score(50, digits=2, logits_rows=2)            # ... grown, and the dumped rows
    seen()
    M.fresh(owner, 30)
    M.fresh(bor, 17)
    owner.prefill_packed([owner, bor], [30, 17], with_logits=True, digits=2)
    assert (owner.position(), bor.position()) == (30, 17)
    seen()
    owner.step_wide([owner, bor], n=1, digits=2)        # the wide_* group
    assert (owner.position(), bor.position()) == (31, 18)
    seen()
    owner.fork_into([bor], 20)                          # the fork tables
    assert bor.position() == 20
    owner.shift(4, 8)
    assert owner.position() == 23
    owner.set_logprobs(2)                               # records + scratch
    bor.set_logprobs(2)
    seen()
    batch.set_slot(0, owner)                            # the batch's buffers
    batch.set_slot(1, bor)
    batch.step(1)
    assert (owner.position(), bor.position()) == (24, 21)
    assert owner.logprob_records(24, 1)["token"][0] >= 0
    seen()
    return peak


@pytest.mark.parametrize("owner_first", [False, True], ids=["owner-last", "owner-handle-first"])
def test_every_allocation_is_freed_exactly_once(pkg, model, owner_first):
    start = pkg.host_device_bytes()
    owner = model.decoder()
    one = pkg.host_device_bytes() - start
    bor = owner.shared()
    two = pkg.host_device_bytes() - start
    assert 0 < two - one < one, "a borrower allocates its own caches and vectors, but no norm vectors"
    batch = pkg.HostBatch(2)
    peak = drive_every_growth_site(model, owner, bor, batch) - start
    print(f"\nDEVBYTES owner {one} owner+borrower {two} peak {peak}")
    assert peak > two
    if owner_first:
        owner.close()  # the handle goes; the borrower and the batch keep the object
        assert pkg.host_device_bytes() - start >= two
        batch.step(1)  # ... and its norm vectors, embedding table and weights
        assert bor.position() == 22
        batch.close()
        assert pkg.host_device_bytes() - start >= two
        bor.close()
    else:
        batch.close()
        bor.close()
        assert one <= pkg.host_device_bytes() - start < peak
        owner.close()
    assert pkg.host_device_bytes() == start


def test_chain_buffers_in_a_child_process(pkg, hip):
    """BITNET_HOST_PREFILL_CHAIN=1 is read by the constructor: the f16 chain's buffers grow and go in a process of their own"""
    env = dict(os.environ, BITNET_HOST_PREFILL_CHAIN="1")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "chain"], capture_output=True, text=True, timeout=240, env=env)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert "CHAIN ok" in run.stdout, run.stdout[-2000:]
    print("\n" + run.stdout.strip().splitlines()[-1])


def chain_child():
    pkg = importlib.import_module("bitnet-rs_amd")
    pkg.load().init(0)
    M = Model(pkg)
    start = pkg.host_device_bytes()
    dec = M.decoder()
    base = pkg.host_device_bytes()
    sizes = []
    for n in (21, 130, 21):
        M.fresh(dec, n)
        dec.prefill(n, with_logits=True, digits=2)
        assert dec.last_prefill_path() == 1, dec.last_prefill_path()
        sizes.append(pkg.host_device_bytes() - base)
    assert sizes[1] > sizes[0] and sizes[2] == sizes[1], sizes  # grows, never shrinks
    dec.close()
    assert pkg.host_device_bytes() == start, (pkg.host_device_bytes(), start)
    print(f"CHAIN ok: prompt buffers {sizes}")


def digest(M, dec):
    h = hashlib.sha256()
    k, v = kv.caches(dec, M.cfg, 0, False)
    n = dec.position()
    assert n > 0
    for a in (dec.last_logits(), dec.last_hidden(), k[:n], v[:n]):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def call_prefill(M, decs, size):
    n = {"small": 21, "large": 130}[size]
    M.fresh(decs[0], n)
    decs[0].prefill(n, with_logits=True, digits=2)


def call_score(M, decs, size):
    n, rows = {"small": (21, 1), "large": (130, 2)}[size]
    M.fresh(decs[0], n)
    res = decs[0].score(n, digits=2, logits_rows=rows)
    assert np.isfinite(res.nll).all() and np.isfinite(res.logits).all()


def call_step_wide(M, decs, size):
    members = decs[:{"small": 1, "large": 3}[size]]
    for i, d in enumerate(members):
        M.fresh(d, 22 + i)
        d.prefill(21 + i, with_logits=False, digits=2)
    decs[0].step_wide(members, n=1, digits=2)
    assert [d.position() for d in members] == [22 + i for i in range(len(members))]


@pytest.mark.parametrize("call", [call_prefill, call_score, call_step_wide], ids=["prefill", "score", "step_wide"])
def test_growth_frees_the_old_group_and_changes_no_result(pkg, model, call):
    def trio():
        base = pkg.host_device_bytes()
        owner = model.decoder()
        decs = [owner, owner.shared(), owner.shared()]
        return base, decs

    base, grown = trio()
    call(model, grown, "small")
    call(model, grown, "large")
    grown_bytes = pkg.host_device_bytes() - base
    call(model, grown, "small")
    assert pkg.host_device_bytes() - base == grown_bytes, "never shrinks"
    got = digest(model, grown[0])
    for d in reversed(grown):
        d.close()
    assert pkg.host_device_bytes() == base

    base, large_only = trio()
    call(model, large_only, "large")
    large_bytes = pkg.host_device_bytes() - base
    for d in reversed(large_only):
        d.close()
    base, small_only = trio()
    call(model, small_only, "small")
    small_bytes = pkg.host_device_bytes() - base
    want = digest(model, small_only[0])
    for d in reversed(small_only):
        d.close()
    print(f"\nGROWTH {call.__name__}: small {small_bytes} large {large_bytes} small+large {grown_bytes}")
    assert grown_bytes == large_bytes, "the grown decoder holds what a decoder that only made the larger call holds: the old group was freed"
    assert small_bytes < large_bytes
    assert got == want, "a call in grown buffers leaves other bytes than the same call in a fresh decoder's"


def test_logprobs_then_reset_at_position_zero(pkg, model):
    dec = model.decoder()
    assert dec.position() == 0
    dec.set_logprobs(2)
    dec.reset()
    recs = dec.logprob_records(0, 4)
    assert (recs["token"] == -1).all()  # cleared to 0xFF bytes: never written
    dec.close()


if __name__ == "__main__":
    if sys.argv[1:] == ["chain"]:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        chain_child()
