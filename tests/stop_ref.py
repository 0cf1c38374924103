"""Plain-Python restatement of the device stop criteria (include/bitnet_hip.h, "stop criteria on the device"): one launch of bitnet_hip_stop_dev
on the words it reads and writes, and a run of launches with the pick's position bump in front of each.  Integers only.

`fault` plants one of FAULTS into the restatement: tests/test_stop_ref.py shows that each is caught by a named case, so the cases the GPU
tests replay are known to tell these mistakes apart."""
from __future__ import annotations

import dataclasses

NONE, TOKEN, EOS, MAX_TOKENS, SEQUENCE = 0, 1, 2, 3, 4
FROZEN_FORCED = 0x7FFFFFFF
MAX_IDS, MAX_SEQS, MAX_SEQ_LEN = 32, 16, 32
FAULTS = ("match_into_prompt", "longest_sequence", "budget_off_by_one", "forced_counted", "position_not_restored", "n_forced_left")


@dataclasses.dataclass
class Config:
    stop_ids: tuple = ()
    eos: int | None = None
    max_tokens: int = 0
    sequences: tuple = ()

    def kwargs(self) -> dict:
        return dict(stop_ids=tuple(self.stop_ids), eos=self.eos, max_tokens=self.max_tokens, sequences=tuple(tuple(s) for s in self.sequences))


@dataclasses.dataclass
class State:
    reason: int = NONE
    index: int = 0
    token: int = 0
    position: int = 0
    generated: int = 0
    frozen_steps: int = 0
    window: int = 0  # not part of bitnet_hip_stop_state: tokens counted since the last arm

    def public(self) -> tuple:
        return (self.reason, self.index, self.token, self.position, self.generated, self.frozen_steps)

    def arm(self, keep_generated: bool = False) -> None:
        g = self.generated if keep_generated else 0
        self.__init__()
        self.generated = g


@dataclasses.dataclass
class Words:
    """the device words of one sequence: *pos, history[capacity], *n_forced, *token (None: a NULL token pointer), the table's live count"""
    pos: int
    history: list
    n_forced: int
    token: int | None = None
    live: int | None = None

    def copy(self) -> "Words":
        return Words(self.pos, list(self.history), self.n_forced, self.token, self.live)


def launch(cfg: Config, st: State, w: Words, capacity: int | None = None, fault: str | None = None) -> None:
    """one bitnet_hip_stop_dev launch"""
    cap = len(w.history) if capacity is None else capacity
    if st.reason != NONE:
        if fault != "position_not_restored":
            w.pos = st.position
        if w.token is not None:
            w.token = st.token
        st.frozen_steps += 1
        return
    P = w.pos
    if P < 1 or P >= cap:
        return
    if P < w.n_forced and fault != "forced_counted":
        return
    t = w.history[P]
    st.generated += 1
    st.window += 1
    reason, index = NONE, 0
    ids = list(cfg.stop_ids)
    budget = cfg.max_tokens + 1 if fault == "budget_off_by_one" else cfg.max_tokens
    if t in ids:
        reason, index = TOKEN, ids.index(t)
    elif cfg.eos is not None and t == cfg.eos:
        reason = EOS
    elif cfg.max_tokens > 0 and st.generated >= budget:
        reason = MAX_TOKENS
    else:
        hits = []
        for s, seq in enumerate(cfg.sequences):
            L = len(seq)
            reach = P + 1 if fault == "match_into_prompt" else st.window
            if L <= reach and P - L + 1 >= 0 and [w.history[i] if i < cap else None for i in range(P - L + 1, P + 1)] == list(seq):
                hits.append(s)
        if hits:
            reason = SEQUENCE
            index = max(hits, key=lambda s: (len(cfg.sequences[s]), -s)) if fault == "longest_sequence" else hits[0]
    if reason == NONE:
        return
    st.reason, st.index, st.token, st.position, st.frozen_steps = reason, index, t, P, 0
    if fault != "n_forced_left":
        w.n_forced = FROZEN_FORCED
    if w.live is not None:
        w.live -= 1


def pick(w: Words, token: int) -> None:
    """what every pick does in front of the stop launch: p = *pos; at a forced position (p + 1 < *n_forced) the history keeps its entry,
    else history[p + 1] = token; *pos = p + 1"""
    p = w.pos
    if not (p + 1 < w.n_forced):
        w.history[p + 1] = token
    w.pos = p + 1
    if w.token is not None:
        w.token = w.history[p + 1]


def run(cfg: Config, st: State, w: Words, tokens, fault: str | None = None) -> list:
    """a run of steps: step i picks tokens[i] (ignored at a forced position), then launches.  Returns the public state after every step."""
    out = []
    for t in tokens:
        pick(w, t)
        launch(cfg, st, w, fault=fault)
        out.append(st.public())
    return out


def first_stop(cfg: Config, history, n_prompt: int, n_steps: int, generated: int = 0):
    """The step k (1-based) at which a generation that placed history[n_prompt .. n_prompt + n_steps) behind an n_prompt-token prompt stops, and
    the state then; (None, state) if it does not stop within n_steps.  Step i places history[n_prompt - 1 + i]... the first generated token
    sits at slot n_prompt (placed by the prompt forward or the last prompt step), so step k places slot n_prompt + k - 1."""
    hist = list(history[:n_prompt]) + [0] * (len(history) - n_prompt)
    w = Words(pos=n_prompt - 1, history=hist, n_forced=n_prompt, token=0)
    st = State(generated=generated)
    for k in range(1, n_steps + 1):
        pick(w, history[n_prompt + k - 1])
        launch(cfg, st, w)
        if st.reason != NONE:
            return k, st
    return None, st
