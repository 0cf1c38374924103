"""numpy restatement of the context shift (bitnet_hip_kv_shift_dev, Decoder::shift; include/bitnet_hip.h, host/decoder.hpp).

shift_f32(k, v, sin, cos, keep, discard, n) works on the [slots, kv, D] arrays tests/extend_ref.py's decode_k / decode_v give, float32 or float16:
slot j takes slot j + discard for every j in [keep, n - discard) -- V as it is, K re-rotated; every other slot keeps its value.  The K arithmetic
is the entry's, operation by operation in float32 (numpy rounds every * and + on its own, the kernel is built with -ffp-contract=off):
for every RoPE pair (x0, x1) = dims (i, i + 64), (sa, ca) = table row j + discard, (sb, cb) = table row j,

    c = ca*cb + sa*sb      s = sa*cb - ca*sb      x0' = x0*c + x1*s      x1' = x1*c - x0*s

An f16 word is widened exactly and the result rounded once (nearest-even).  The device result must equal this BIT FOR BIT.

THE BOUND.  What a prompt forward would write at slot j is the raw key (r0, r1) rotated by table row j; target_f64 computes that in float64 from the
f32 table values.  With u = 2^-24 and N = |k0| + |k1| (>= the pair's 2-norm, which every rotation preserves), to first order in u:
  1. the stored key's own rounding.  It was written as fl(fl(r0 ca) - fl(r1 sa)), fl(fl(r0 sa) + fl(r1 ca)): each component is off by at most
     u (|r0 ca| + |r1 sa|) + u |k0| <= 2 u ||r||_2; rotated by (c, s) that is at most 2 u ||r||_2 (|c| + |s|) <= 2 sqrt(2) u N.
  2. c and s.  c = fl(fl(ca cb) + fl(sa sb)) is off by at most u (|ca cb| + |sa sb|) + u |c| <= 2 u, and so is s; the result moves by
     |k0| 2u + |k1| 2u = 2 u N (<= 2 sqrt(2) u N).
  3. the final rotation.  fl(fl(k0 c) + fl(k1 s)) is off by at most u (|k0 c| + |k1 s|) + u |x0'| <= 2 u ||k||_2 (<= 2 sqrt(2) u N).
  4. (not in the issue's list) the table rows are not exactly unit vectors.  In exact arithmetic the formula gives (sa^2 + ca^2) times the target:
     the two rows compose to a rotation only up to row a's norm.  With correctly rounded table entries |sa^2 + ca^2 - 1| <= 2 u: at most
     2 u ||k||_2.
  Terms 1 to 3 are each at most 2 sqrt(2) u N, the issue's 9 u N = 3 * 2 sqrt(2) u N rounded up; counted as above (2 sqrt(2) + 2 + 2 + 2 with term
  4) the sum is 8.83 u N, inside the same 9 u N, the rest being room for the second-order terms.  BOUND_UNITS = 9.
  An f16 cache adds the one rounding of the result: 2^-11 |value| + 2^-25 (half an ulp of a normal value, half the subnormal spacing).
Observed on standard-normal keys (tests/test_shift_ref.py): about 4 u N; rotating by table row `discard` instead is off by thousands of u N.

Also the host-side arithmetic of Decoder::shift as pure functions: shift_state (position, forced count, history) and shift_records.
"""
from __future__ import annotations

import numpy as np

D = 128
HALF = D // 2
U = 2.0 ** -24
BOUND_UNITS = 9.0


def rope_tables(max_pos, theta):
    """The decoder's tables (host/decoder.cpp, as crates/bitnet-rope/src/lib.rs:59-93): inv[i] = 1 / theta^(2 i / D), angle = (float) p * inv[i] in
    f32, then the sine and cosine of that f32 angle, here correctly rounded (float64 libm, rounded once)."""
    inv = (np.float32(1.0) / np.power(np.float32(theta), (np.float32(2.0) * np.arange(HALF, dtype=np.float32)) / np.float32(D))).astype(np.float32)
    angle = (np.arange(max_pos, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float32)
    a64 = angle.astype(np.float64)
    return np.sin(a64).astype(np.float32), np.cos(a64).astype(np.float32)


def rerotate_f32(x, sa, ca, sb, cb):
    """x: [m, kv, D] float32; sa, ca, sb, cb: [m, 64] float32 -> [m, kv, D] float32, the formula above"""
    f = np.float32
    sa, ca, sb, cb = (np.asarray(t, f)[:, None, :] for t in (sa, ca, sb, cb))
    c = (ca * cb + sa * sb).astype(f)
    s = (sa * cb - ca * sb).astype(f)
    x0, x1 = x[..., :HALF], x[..., HALF:]
    return np.concatenate([(x0 * c + x1 * s).astype(f), (x1 * c - x0 * s).astype(f)], axis=-1)


def shift_f32(k, v, sin, cos, keep, discard, n):
    """-> (k', v'): copies of the [slots, kv, D] arrays with slots [keep, n - discard) replaced; dtype float32 or float16 as given"""
    k2, v2 = np.array(k, copy=True), np.array(v, copy=True)
    j = np.arange(keep, n - discard)
    if j.size:
        v2[j] = v[j + discard]
        sin, cos = np.asarray(sin, np.float32).reshape(-1, HALF), np.asarray(cos, np.float32).reshape(-1, HALF)
        with np.errstate(all="ignore"):
            k2[j] = rerotate_f32(np.asarray(k[j + discard], np.float32), sin[j + discard], cos[j + discard], sin[j], cos[j]).astype(k.dtype)
    return k2, v2


def rotate_f64(r, sin_rows, cos_rows):
    """raw keys [m, kv, D] rotated by the given table rows [m, 64] in float64 (split-half RoPE, extend_ref.rope_np)"""
    r = np.asarray(r, np.float64)
    s, c = np.asarray(sin_rows, np.float64)[:, None, :], np.asarray(cos_rows, np.float64)[:, None, :]
    r0, r1 = r[..., :HALF], r[..., HALF:]
    return np.concatenate([r0 * c - r1 * s, r0 * s + r1 * c], axis=-1)


def unrotate_f64(k, sin_rows, cos_rows):
    """the raw keys whose rotation by the given table rows is EXACTLY k: the inverse of the table's 2 x 2 matrix (not its transpose: the rows
    are unit vectors only up to rounding)"""
    k = np.asarray(k, np.float64)
    s, c = np.asarray(sin_rows, np.float64)[:, None, :], np.asarray(cos_rows, np.float64)[:, None, :]
    k0, k1 = k[..., :HALF], k[..., HALF:]
    det = c * c + s * s
    return np.concatenate([(k0 * c + k1 * s) / det, (k1 * c - k0 * s) / det], axis=-1)


def target_f64(raw, sin, cos, keep, discard, n):
    """raw: [slots, kv, D] raw keys BY SOURCE SLOT -> the keys a prompt forward would write at slots [keep, n - discard): [m, kv, D] float64"""
    j = np.arange(keep, n - discard)
    return rotate_f64(np.asarray(raw)[j + discard], sin[j], cos[j])


def bound(target, f16=False):
    """per element of target [m, kv, D]: BOUND_UNITS u (|k0| + |k1|) of its pair (+ the f16 rounding)"""
    t = np.abs(np.asarray(target, np.float64))
    pair = t[..., :HALF] + t[..., HALF:]
    b = BOUND_UNITS * U * np.concatenate([pair, pair], axis=-1)
    return b + (2.0 ** -11 * t + 2.0 ** -25 if f16 else 0.0)


def shift_forced(f, keep, discard):
    return f if f <= keep else keep if f <= keep + discard else f - discard


def shift_state(pos, forced, history, keep, discard, max_pos):
    """-> (position, forced count, history) after Decoder::shift(keep, discard).  history: the max_pos + 2 entries the decoder holds (or fewer:
    entries beyond the array are taken as absent).  Entries [keep + discard, max_pos) move down by discard, zero beyond."""
    h = np.asarray(history, np.int32)
    out = np.zeros_like(h)
    out[:keep] = h[:keep]
    src = np.arange(keep + discard, min(max_pos, h.size))
    out[src - discard] = h[src]
    return pos - discard, shift_forced(forced, keep, discard), out


def shift_records(records, pos, keep, discard):
    """records: any array with one entry per position -> after the shift: record q <= keep stays, record q in (keep, pos - discard] is the old
    record q + discard, every record above the new last one (pos - discard) is 0xFF bytes"""
    r = np.ascontiguousarray(records)
    out = r.copy()
    out.view(np.uint8).reshape(r.shape[0], -1)[keep + 1:] = 0xFF
    q = np.arange(keep + 1, pos - discard + 1)
    out[q] = r[q + discard]
    return out
