#!/usr/bin/env python3
"""Records the reference's dequantize_row_iq2_s (crates/bitnet-ggml-ffi/csrc/ggml/src/ggml-quants.c:59-72) on the blocks
tests/test_oracle_kat.py::test_vendored_ggml_pins_lut_and_bit_order checks, so the test runs without the reference tree.
Needs oracle/_ref/libggml_iq2s_ref.so (oracle.build() compiles it where the reference tree is present).

    python tests/golden/make_iq2s_ref_fixture.py     # writes tests/golden/iq2s_ref_dequant.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# block 0: f16 1.0 over the byte 0xE4 (codes 0, 1, 2, 3 LSB first); then eight scales over random bytes of default_rng(7)
D_BITS = (0x3C00, 0x3C00, 0x4000, 0x3555, 0x2E66, 0x0400, 0x03FF, 0x0001, 0x5640)


def blocks():
    rng = np.random.default_rng(7)
    qs = [np.full(64, 0xE4, np.uint8)] + [rng.integers(0, 256, 64, dtype=np.uint8) for _ in D_BITS[1:]]
    return np.array(D_BITS, np.uint16), np.stack(qs)


def main():
    from oracle import oracle as orc

    orc.build()
    if not orc.ref_available():
        sys.exit("oracle/_ref/libggml_iq2s_ref.so is not built (the reference tree is absent)")
    d, qs = blocks()
    y = np.stack([orc.ref_dequantize_row_iq2_s(int(b), q) for b, q in zip(d, qs)])
    np.savez(os.path.join(HERE, "iq2s_ref_dequant.npz"), d_bits=d, qs=qs, y=y)


if __name__ == "__main__":
    main()
