"""numpy restatement of bitnet_hip_attention_extend_dev (include/bitnet_hip.h): seq_len new tokens at absolute positions
past .. past + seq_len - 1 attend over the keys 0 .. own position, the first `past` of which come from the cache
(the reference: seq_len queries over past_len + seq_len keys, create_causal_mask(q_len, k_len), T:455-470, T:704-719; cache
append T:1171-1202).  Everything in float64; split-half RoPE as tests/test_prefill_parity.py::rope_np.

Also encode / decode of the library's four private cache layouts (kernels_attn.hip), per KV head padded to whole 64-position
chunks C = ceil(max_pos / 64):
  K f32  [kv][C][D][64]             element (d, pos) at ((pos // 64) * D + d) * 64 + pos % 64
  K f16  [kv][C][D / 2][64][2]      element (d, pos) at (((pos // 64) * D / 2 + d // 2) * 64 + pos % 64) * 2 + d % 2
  V f32 / f16  [kv][C * 64][D]
"""
from __future__ import annotations

import numpy as np

D = 128


def rope_np(x, sin, cos):
    half = x.shape[-1] // 2
    x0, x1 = x[..., :half], x[..., half:]
    return np.concatenate([x0 * cos - x1 * sin, x0 * sin + x1 * cos], axis=-1)


def split_qkv(qkv, n_heads, n_kv):
    """[n, (heads + 2 kv) * D] -> q [n, heads, D], k [n, kv, D], v [n, kv, D] (float64)"""
    n = qkv.shape[0]
    q = qkv[:, : n_heads * D].reshape(n, n_heads, D).astype(np.float64)
    k = qkv[:, n_heads * D:(n_heads + n_kv) * D].reshape(n, n_kv, D).astype(np.float64)
    v = qkv[:, (n_heads + n_kv) * D:].reshape(n, n_kv, D).astype(np.float64)
    return q, k, v


def extend_f64(qkv_new, k_past, v_past, n_heads, n_kv, sin, cos):
    """One continuation.  qkv_new: [n, (heads + 2 kv) * D] raw projections of the new tokens; k_past (rotated) / v_past: [past, kv, D];
    sin / cos: [max_pos, D / 2].  -> (out [n, heads, D], k_all [past + n, kv, D] rotated, v_all [past + n, kv, D])."""
    past, n = k_past.shape[0], qkv_new.shape[0]
    pos = np.arange(past, past + n)
    q, k, v = split_qkv(qkv_new, n_heads, n_kv)
    q = rope_np(q, sin[pos, None, :], cos[pos, None, :])
    k = rope_np(k, sin[pos, None, :], cos[pos, None, :])
    k_all = np.concatenate([np.asarray(k_past, np.float64).reshape(past, n_kv, D), k])
    v_all = np.concatenate([np.asarray(v_past, np.float64).reshape(past, n_kv, D), v])
    group = n_heads // n_kv
    hidden = np.arange(past + n)[None, :] > pos[:, None]  # key j is hidden from query i when j > past + i
    out = np.zeros((n, n_heads, D))
    for h in range(n_heads):
        s = q[:, h] @ k_all[:, h // group].T / np.sqrt(D)
        s[hidden] = -np.inf
        pm = np.exp(s - s.max(axis=1, keepdims=True))
        out[:, h] = (pm / pm.sum(axis=1, keepdims=True)) @ v_all[:, h // group]
    return out, k_all, v_all


def causal_f64(qkv, n_heads, n_kv, sin, cos):
    """The one-shot prompt: all rows of qkv from position 0."""
    return extend_f64(qkv, np.zeros((0, n_kv, D)), np.zeros((0, n_kv, D)), n_heads, n_kv, sin, cos)


def chunks(max_pos):
    return (max_pos + 63) // 64


def _padded(x, max_pos):
    """[T, kv, D] -> [C, 64, kv, D] with zeros beyond T"""
    T, n_kv, _ = x.shape
    C = chunks(max_pos)
    full = np.zeros((C * 64, n_kv, D), x.dtype)
    full[:T] = x
    return full.reshape(C, 64, n_kv, D)


def encode_k(k, max_pos, f16=False):
    """rotated keys [T, kv, D] -> the flat K cache (float32 or float16), zeros beyond T"""
    p = _padded(np.asarray(k, np.float16 if f16 else np.float32), max_pos)
    if f16:
        C, _, n_kv, _ = p.shape
        return np.ascontiguousarray(p.reshape(C, 64, n_kv, D // 2, 2).transpose(2, 0, 3, 1, 4)).reshape(-1)
    return np.ascontiguousarray(p.transpose(2, 0, 3, 1)).reshape(-1)


def decode_k(flat, n_kv, max_pos, f16=False):
    """the flat K cache -> [C * 64, kv, D]"""
    C = chunks(max_pos)
    if f16:
        a = np.asarray(flat, np.float16).reshape(n_kv, C, D // 2, 64, 2).transpose(1, 3, 0, 2, 4)
        return np.ascontiguousarray(a).reshape(C * 64, n_kv, D)
    return np.ascontiguousarray(np.asarray(flat, np.float32).reshape(n_kv, C, D, 64).transpose(1, 3, 0, 2)).reshape(C * 64, n_kv, D)


def encode_v(v, max_pos, f16=False):
    p = _padded(np.asarray(v, np.float16 if f16 else np.float32), max_pos)
    C, _, n_kv, _ = p.shape
    return np.ascontiguousarray(p.reshape(C * 64, n_kv, D).transpose(1, 0, 2)).reshape(-1)


def decode_v(flat, n_kv, max_pos, f16=False):
    C = chunks(max_pos)
    return np.ascontiguousarray(np.asarray(flat, np.float16 if f16 else np.float32).reshape(n_kv, C * 64, D).transpose(1, 0, 2))


def k_index(d, pos, f16=False):
    """flat index of element (d, pos) inside ONE KV head of the K cache"""
    if f16:
        return (((pos // 64) * (D // 2) + d // 2) * 64 + pos % 64) * 2 + d % 2
    return ((pos // 64) * D + d) * 64 + pos % 64
