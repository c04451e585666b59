"""Quantization round-trip tests.

Mirrors the reference test strategy (src/nn/nn-cpu-ops-test.cpp:87-104):
Q40/Q80 quantize<->dequantize round-trips with the same tolerances
(0.13 absolute for Q40 on [-1,1]-ish data scaled, 0.01 for Q80).
"""

import numpy as np
import pytest

from dllama_amd import quants


def test_q80_roundtrip():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(4096).astype(np.float32)) * 2
    y = quants.q80_roundtrip(x)
    # reference tolerance: 0.01 on k/nBlocks-scaled ramp; scale-relative here
    assert np.abs(x - y).max() <= np.abs(x).max() / 127.0 * 1.01


def test_q40_roundtrip():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(4096).astype(np.float32)
    y = quants.q40_roundtrip(x)
    # Q40 is 4-bit: block-absmax/8 max error plus rounding slack
    assert np.abs(x - y).max() <= np.abs(x).max() / 8.0 * 1.2


def test_q40_block_layout():
    # byte j of a block must hold elem j (lo nibble) and elem j+16 (hi nibble)
    x = np.arange(32, dtype=np.float32) - 16
    b = quants.quantize_q40(x)
    assert b.shape == (1, 18)
    d = b[0, :2].copy().view(np.float16).astype(np.float32)[0]
    lo = (b[0, 2:] & 0xF).astype(np.int32) - 8
    hi = ((b[0, 2:] >> 4) & 0xF).astype(np.int32) - 8
    recon = np.concatenate([lo, hi]) * d
    assert np.abs(recon - x).max() <= np.abs(x).max() / 8.0 * 1.2


def test_q80_zeros():
    x = np.zeros(64, dtype=np.float32)
    y = quants.q80_roundtrip(x)
    assert np.all(y == 0)


def test_q40_planes():
    rng = np.random.default_rng(2)
    d_rows, n_cols = 8, 96
    w = rng.standard_normal((d_rows, n_cols)).astype(np.float32)
    blocks = quants.quantize_q40(w)
    qs, scales = quants.q40_to_planes(blocks, d_rows, n_cols)
    assert qs.shape == (d_rows, n_cols // 2)
    assert scales.shape == (d_rows, n_cols // 32)
    # reconstruct from planes and compare to block dequant
    ref = quants.dequantize_q40(blocks, d_rows * n_cols).reshape(d_rows, n_cols)
    lo = (qs & 0xF).astype(np.int8) - 8
    hi = (qs >> 4).astype(np.int8) - 8
    nb = n_cols // 32
    vals = np.empty((d_rows, n_cols), dtype=np.float32)
    for b in range(nb):
        vals[:, b * 32: b * 32 + 16] = lo[:, b * 16:(b + 1) * 16]
        vals[:, b * 32 + 16:(b + 1) * 32] = hi[:, b * 16:(b + 1) * 16]
    vals *= np.repeat(scales.astype(np.float32), 32, axis=1)
    assert np.allclose(vals, ref)


def test_quantizers_byte_exact_vs_reference_converter(tmp_path):
    """Require byte-identical Q40 and Q80 output to the reference's OWN
    Python converter (converter/writer.py: writeQuantizedQ40Tensor /
    writeQuantizedQ80Tensor) on the same data — pins the wire format beyond
    the layout unit tests. tests/golden/quant_input_f32.npy is the input the
    reference converter was run on, quant_ref_q40.bin / quant_ref_q80.bin
    are the bytes it wrote."""
    import os

    import numpy as np

    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    x = np.load(os.path.join(golden, "quant_input_f32.npy"))
    assert x.dtype == np.float32 and x.shape == (2048,)
    # the input is the seeded draw it always was, incl. the all-zero block
    rng = np.random.default_rng(17)
    want = (rng.standard_normal(2048) * 0.7).astype(np.float32)
    want[:32] = 0.0
    assert np.array_equal(x, want)

    with open(os.path.join(golden, "quant_ref_q40.bin"), "rb") as f:
        ref_q40 = f.read()
    assert len(ref_q40) == 2048 // 32 * 18
    assert ref_q40 == quants.quantize_q40(x).tobytes()

    with open(os.path.join(golden, "quant_ref_q80.bin"), "rb") as f:
        ref_q80 = f.read()
    assert len(ref_q80) == 2048 // 32 * 34
    assert ref_q80 == quants.quantize_q80(x).tobytes()
