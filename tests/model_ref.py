"""numpy restatement of the whole-prompt forward in float64: oracle/transformer_oracle.c::bo_model_step over all n rows at once.

  embedding (the f16 row gather) -> per layer: LayerNorm (mean-subtracting, eps inside the root) -> q | k | v -> split-half RoPE + causal
  attention (extend_ref.causal_f64, which also returns the rotated K and the V: what a KV cache must hold) -> o-projection + residual ->
  LayerNorm -> silu(gate) * up -> down-projection + residual; final LayerNorm -> the tied head.

One hook, `rnd`: a function applied to the four activations that feed a matmul (the two LayerNorm outputs, the attention output and
silu * up).  rnd=None is the reference; rnd=f16 is the F16-ACTIVATION CLASS MODEL: the same forward with those four hand-overs rounded once
to f16, the coarsest rounding any device path applies to them.  Its distance from the reference is the yardstick the decoder's caches are
held to (tests/test_decoder_state_gpu.py), computed from the reference alone.

RoPE tables come from the caller (oracle.rope_tables: the f32 tables are part of the model's definition, the device holds the same ones).
"""
from __future__ import annotations

import collections

import numpy as np

import extend_ref as er

PROJ = ("q", "k", "v", "o", "gate", "up", "down")
TERNARY = np.array([0.0, 1.0, 0.0, -1.0])    # BitNet32 code map (oracle: tern_value)
QK256 = np.array([-2.0, -1.0, 1.0, 2.0])     # oracle: code_to_f32; unpack_qk256_block: byte i of a 64-byte block holds elements 4 i .. 4 i + 3, low bits first

Forward = collections.namedtuple("Forward", "K V resid logits")


def f16(a):
    """round-to-nearest-even to f16, back in float64"""
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def _codes(packed, rows, cols):
    pk = np.asarray(packed, np.uint8).reshape(rows, -1)
    return np.stack([(pk >> (2 * i)) & 3 for i in range(4)], axis=-1).reshape(rows, -1)[:, :cols]


def dense_weights(cfg, layer, fmt):
    """synth.make_layer output -> {projection: float64 [out, in]} + the two gammas"""
    d = {"attn_norm": np.asarray(layer["attn_norm"], np.float64), "ffn_norm": np.asarray(layer["ffn_norm"], np.float64)}
    for name, (rows, cols) in cfg.shapes().items():
        if fmt == "qk256":
            assert cols % 256 == 0
            d[name] = QK256[_codes(layer[name], rows, cols)]
        else:
            s = np.asarray(layer[name + "_scales"], np.float64).reshape(rows, cols // 32)
            d[name] = TERNARY[_codes(layer[name], rows, cols)] * np.repeat(s, 32, axis=1)
    return d


def layernorm(x, gamma, eps):
    d = x - x.mean(axis=-1, keepdims=True)
    return d / np.sqrt((d * d).mean(axis=-1, keepdims=True) + eps) * gamma


def forward(cfg, dense, glob, tokens, sin, cos, rnd=None):
    """dense: [dense_weights(...)] per layer; sin / cos: [max_pos, D / 2].  -> Forward(K [L][n, kv, D] rotated, V [L][n, kv, D], resid [L, n, hidden]
    the residual stream after each block, logits [n, vocab])"""
    rnd = rnd or (lambda a: a)
    sin, cos = np.asarray(sin, np.float64).reshape(-1, er.D // 2), np.asarray(cos, np.float64).reshape(-1, er.D // 2)
    tokens = np.asarray(tokens, np.int64)
    n = tokens.size
    assert cfg.head_dim == er.D
    emb = np.asarray(glob["embed_f16"], np.uint16).view(np.float16).reshape(cfg.vocab, cfg.hidden)
    x = emb[tokens].astype(np.float64)
    K, V, resid = [], [], []
    for w in dense:
        xn = rnd(layernorm(x, w["attn_norm"], cfg.eps))
        qkv = np.concatenate([xn @ w["q"].T, xn @ w["k"].T, xn @ w["v"].T], axis=1)
        att, k, v = er.causal_f64(qkv, cfg.n_heads, cfg.n_kv_heads, sin, cos)
        K.append(k)
        V.append(v)
        x = rnd(att.reshape(n, -1)) @ w["o"].T + x
        xn = rnd(layernorm(x, w["ffn_norm"], cfg.eps))
        g, u = xn @ w["gate"].T, xn @ w["up"].T
        x = rnd(g / (1.0 + np.exp(-g)) * u) @ w["down"].T + x
        resid.append(x)
    hn = layernorm(x, np.asarray(glob["final_norm"], np.float64), cfg.eps)
    return Forward(K, V, np.stack(resid), hn @ emb.astype(np.float64).T)


def kv_rel(got, want):
    """per (position, kv head): ||got - want||_2 / ||want||_2 over the D elements; got / want [n, kv, D]"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.linalg.norm(got - want, axis=-1) / np.linalg.norm(want, axis=-1)


def yardstick(ref, cls):
    """u_l: per layer the largest kv_rel of the class model's K and V rows against the reference's"""
    return [max(float(kv_rel(cls.K[l], ref.K[l]).max()), float(kv_rel(cls.V[l], ref.V[l]).max())) for l in range(len(ref.K))]
