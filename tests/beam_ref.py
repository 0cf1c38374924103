"""numpy restatement of the beam search rule (include/bitnet_hip_beam.h; csrc/beam_rule.hpp is the compiled statement): every float operation is one
float32 operation in the stated order.  BeamRef holds the state words of bitnet_hip_beam_state under the same names; step() takes per beam the
tap record's lse and its first 2B (id, logit) pairs and the cache slot p the step filled; select() is what bitnet_hip_beam_select_dev leaves in the
members' positions and histories around it; words() flattens the state for an equality with the device's or the stand-alone program's."""
from __future__ import annotations

import numpy as np

BEAM_MAX = 8
DONE_POOL, DONE_BUDGET, ERR_RANGE, ERR_SHORT = 1, 2, 0x100, 0x200
NEG_INF = np.float32(-np.inf)


def len_weights(max_new: int, alpha: float) -> np.ndarray:
    """the table a caller would pass: len^-alpha in float64, rounded once (entry 0 is never read: 1)"""
    w = np.ones(max_new + 1, np.float64)
    w[1:] = np.arange(1, max_new + 1, dtype=np.float64) ** (-float(alpha))
    return w.astype(np.float32)


def bits(x) -> int:
    return int(np.asarray(x, np.float32).view(np.uint32))


class BeamRef:
    # planted faults for the tests that show a named case catches each (tests/test_beam_ref.py); all off in the rule
    TIE_REVERSED = False  # ties by DEscending candidate index
    FROM_NEW = False      # from[b] taken from div AFTER the step
    EOS_SLACK = 0         # an EOS candidate at walk index B + EOS_SLACK - 1 still pooled

    def __init__(self, n_beams: int, eos: int, max_new: int, len_weight, prompt_pos: int = 0):
        assert n_beams >= 1 and max_new >= 1
        self.cap = max(BEAM_MAX, n_beams)  # the device's state holds BEAM_MAX beams; the restatement takes any number (words() needs <= BEAM_MAX)
        self.n_beams, self.eos, self.max_new = n_beams, eos, max_new
        self.len_weight = np.asarray(len_weight, np.float32).copy()
        assert self.len_weight.size == max_new + 1
        self.reset(prompt_pos)

    def reset(self, P: int):
        self.prompt_pos, self.gen_len, self.done, self.stepped, self.n_slots = P, 0, 0, 0, P
        self.pool_n = self.pool_seq = self.frozen_steps = 0
        self.score = np.full(self.cap, NEG_INF, np.float32)
        self.score[0] = 0.0
        self.parent = np.arange(self.cap, dtype=np.int32)
        self.frm = np.full(self.cap, P, np.int32)
        self.token = np.full(self.cap, -1, np.int32)
        self.div = np.full((self.cap, self.cap), P, np.int32)
        self.pool_score = np.zeros(self.cap, np.float32)
        self.pool_key = np.zeros(self.cap, np.float32)
        self.pool_len = np.zeros(self.cap, np.int32)
        self.pool_order = np.zeros(self.cap, np.int32)
        self.pool_src = np.full(self.cap, -1, np.int32)
        self.pool_last = np.full(self.cap, -1, np.int32)
        self.pool_tokens = [[] for _ in range(self.cap)]
        self.beam_tokens = [[] for _ in range(self.cap)]  # the generated tokens of every live beam (the histories behind prompt_pos)
        self.events = []                                  # what the last step did, for tests that assert a case occurred

    # ---- the rule ----
    def _pool_add(self, score, length, src, last, tokens):
        B = self.n_beams
        with np.errstate(invalid="ignore", over="ignore"):
            key = np.float32(score) * self.len_weight[length]
        if np.isnan(key):
            key = NEG_INF
        if self.pool_n < B:
            slot = self.pool_n
            self.pool_n += 1
            self.events.append(("pool_add", slot))
        else:
            slot = 0
            for i in range(1, B):
                if self.pool_key[i] < self.pool_key[slot] or (self.pool_key[i] == self.pool_key[slot] and self.pool_order[i] > self.pool_order[slot]):
                    slot = i
            if not key > self.pool_key[slot]:
                self.events.append(("pool_drop", slot))
                return
            self.events.append(("pool_replace", slot))
        self.pool_score[slot], self.pool_key[slot], self.pool_len[slot], self.pool_order[slot] = score, key, length, self.pool_seq
        self.pool_seq += 1
        self.pool_src[slot], self.pool_last[slot] = src, last
        self.pool_tokens[slot] = list(tokens)

    def candidates(self, lse, top_id, top_logit):
        """-> (scores f32, order): candidate i = b * W + j, W = width(); order = the indices in walk order"""
        B = self.n_beams
        lse = np.asarray(lse, np.float32)
        top_logit = np.asarray(top_logit, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            lp = top_logit[:B, :self.width(top_logit)] - lse[:B, None]
            cs = (self.score[:B, None] + lp).astype(np.float32).reshape(-1)
        cs = np.where(np.isnan(cs) | (cs == NEG_INF), NEG_INF, cs).astype(np.float32)
        tie = -1 if self.TIE_REVERSED else 1
        order = sorted(range(cs.size), key=lambda i: (-float(cs[i]), tie * i))  # -(-inf) = +inf sorts last; ties by index
        return cs, order

    def width(self, top_logit):
        """candidates per beam: 2B, or the whole row where a tiny vocabulary has fewer entries"""
        return min(2 * self.n_beams, np.asarray(top_logit).shape[1])

    def step(self, lse, top_id, top_logit, p: int):
        B = self.n_beams
        top_id = np.asarray(top_id, np.int32)
        self.events = []
        cs, order = self.candidates(lse, top_id, top_logit)
        W = self.width(top_logit)
        self.walk = [(int(i), int(i) // W, int(i) % W) for i in order[:2 * B]]
        self.pool_src[:] = -1
        self.pool_last[:] = -1
        old_tokens = [list(t) for t in self.beam_tokens]
        ns, npar, ntok = [], [], []
        for r, (i, b, j) in enumerate(self.walk):
            tok = int(top_id[b, j])
            if self.eos >= 0 and tok == self.eos:
                if r < B + self.EOS_SLACK:
                    self.events.append(("eos_pooled", r))
                    self._pool_add(cs[i], self.gen_len + 1, b, tok, old_tokens[b] + [tok])
                else:
                    self.events.append(("eos_skipped", r))
                continue
            if len(ns) < B:
                ns.append(cs[i]), npar.append(b), ntok.append(tok)
        while len(ns) < B:
            nb = len(ns)
            ns.append(NEG_INF), npar.append(nb), ntok.append(-1)
            self.done |= ERR_SHORT
        old_div = self.div.copy()
        for b in range(B):
            for c in range(B):
                self.div[b, c] = p + 1 if npar[b] == npar[c] else old_div[npar[b], npar[c]]
        for b in range(B):
            self.frm[b] = (self.div if self.FROM_NEW else old_div)[b, npar[b]]
        for b in range(B):
            self.score[b], self.parent[b], self.token[b] = ns[b], npar[b], ntok[b]
            self.beam_tokens[b] = old_tokens[npar[b]] + [ntok[b]]
        self.gen_len += 1
        self.n_slots = p + 1
        self.stepped = 1
        if self.pool_n >= B:
            self.done |= DONE_POOL
        elif self.gen_len >= self.max_new:
            for b in range(B):
                self._pool_add(self.score[b], self.gen_len, int(self.parent[b]), int(self.token[b]), self.beam_tokens[b])
            self.done |= DONE_BUDGET

    # ---- what bitnet_hip_beam_select_dev does around the rule ----
    def select(self, records, pos, hist, capacity):
        """records(b, q) -> (lse, top_id[>= 2B], top_logit[>= 2B]) of beam b's record q; pos: int array [B], hist: int array [B][>= capacity]; both
        are modified in place as the launch modifies the device's."""
        B = self.n_beams
        if self.done:
            for b in range(B):
                if pos[b] >= 1:
                    pos[b] -= 1
            self.stepped = 0
            self.frozen_steps += 1
            return
        q = int(pos[0])
        cap = capacity if np.ndim(capacity) else [capacity] * B
        ok = all(int(pos[b]) == q for b in range(B)) and all(1 <= q < int(cap[b]) for b in range(B)) and q - 1 == self.prompt_pos + self.gen_len
        if not ok:
            self.done |= ERR_RANGE
            self.stepped = 0
            return
        p = q - 1
        recs = [records(b, q) for b in range(B)]
        self.step([r[0] for r in recs], np.array([np.asarray(r[1])[:2 * B] for r in recs]), np.array([np.asarray(r[2])[:2 * B] for r in recs]), p)
        old = np.array(hist, copy=True)
        for b in range(B):
            if self.parent[b] != b:
                hist[b][self.frm[b]:p + 1] = old[self.parent[b]][self.frm[b]:p + 1]
            if self.token[b] >= 0:
                hist[b][p + 1] = self.token[b]

    # ---- views ----
    def words(self):
        """every word of bitnet_hip_beam_state, floats as their bits, in the struct's order"""
        assert self.cap == BEAM_MAX
        f = lambda a: [int(x) for x in np.asarray(a, np.float32).view(np.uint32)]
        i = lambda a: [int(x) for x in np.asarray(a).reshape(-1)]
        return ([self.n_beams, self.eos, self.max_new, self.prompt_pos, self.gen_len, self.done, self.stepped, self.n_slots, self.pool_n, self.pool_seq,
                 self.frozen_steps, 0] + f(self.score) + i(self.parent) + i(self.frm) + i(self.token) + i(self.div) + f(self.pool_score) + f(self.pool_key)
                + i(self.pool_len) + i(self.pool_order) + i(self.pool_src) + i(self.pool_last))

    def hypotheses(self):
        """the pool sorted by descending key, then insertion order: [(tokens, score bits, key bits)]"""
        idx = sorted(range(self.pool_n), key=lambda s: (-float(self.pool_key[s]), int(self.pool_order[s])))
        return [(list(self.pool_tokens[s]), bits(self.pool_score[s]), bits(self.pool_key[s])) for s in idx]


STATE_WORDS = 12 + 4 * 8 + 64 + 6 * 8
