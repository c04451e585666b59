"""Synthetic fixtures: byte-level tokenizer + tiny models for tests/demos
(no network: real checkpoints cannot be downloaded in this environment)."""

from __future__ import annotations

from .. import tokenizer as tok
from .. import model_file as mf


def natural_q40_planes(d: int, n: int, seed: int):
    """Gaussian weights (std 0.1) through quants.quantize_q40 -> device-layout
    planes (qs uint8 [d, n/2], scales f16 [d, n/32]) as CPU tensors."""
    import numpy as np
    import torch
    from .. import quants
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((d, n)).astype(np.float32) * 0.1
    qs, sc = quants.q40_to_planes(quants.quantize_q40(w), d, n)
    return torch.from_numpy(qs), torch.from_numpy(sc)


def adversarial_q40_q80(d: int, n: int, rows: int, seed: int):
    """Hand-built Q40 planes and Q80 triple at the corners the quantisers
    rarely reach; no kernel in the loop. CPU tensors
    (qs, scales, xq, xs, xbs):
      qs      uniform random bytes, one weight row all 0x00 (every nibble
              -8) and one all 0xFF (every nibble +7)
      scales  f16, random sign, magnitude 2^U[-10,-3]
      xq      codes uniform in [-127, 127] (-128 never: the quantiser cannot
              emit it); per input row one block all +127, one all -127 and
              one all zero whose scale is 0, where the row has that many
      xs      uniform in [2^-8, 2^-2]
      xbs     the exact code sum"""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    nb = n // 32
    qs = rng.integers(0, 256, (d, n // 2), dtype=np.uint8)
    r0 = int(rng.integers(0, d))
    qs[r0] = 0x00
    if d > 1:
        qs[(r0 + 1 + int(rng.integers(0, d - 1))) % d] = 0xFF
    mag = np.exp2(rng.uniform(-10.0, -3.0, (d, nb)))
    sc = (mag * rng.choice([-1.0, 1.0], (d, nb))).astype(np.float16)
    xq = rng.integers(-127, 128, (rows, nb, 32)).astype(np.int8)
    xs = rng.uniform(2.0 ** -8, 2.0 ** -2, (rows, nb)).astype(np.float32)
    for r in range(rows):
        special = rng.permutation(nb)[:3]
        for j, fill in zip(special, (127, -127, 0)):
            xq[r, j] = fill
            if fill == 0:
                xs[r, j] = 0.0
    xbs = xq.astype(np.int32).sum(-1).astype(np.float32)
    return (torch.from_numpy(qs), torch.from_numpy(sc),
            torch.from_numpy(xq.reshape(rows, n)), torch.from_numpy(xs),
            torch.from_numpy(xbs))


def make_byte_tokenizer(path: str, chat_template: str | None = None) -> None:
    """A byte-level BPE tokenizer: 256 byte tokens, a few merges, and
    llama3-style special tokens. Good enough to exercise the full
    encode -> decode -> chat-template -> eos pipeline."""
    vocab: list[bytes] = [bytes([i]) for i in range(256)]
    scores = [0.0] * 256
    merges = [b"th", b"he", b"the", b" the", b"in", b"an", b"and", b" a",
              b"hello", b" world", b"ll", b"lo", b"wor", b"ld"]
    for i, m in enumerate(merges):
        vocab.append(m)
        scores.append(1.0 + i)  # later merges win ties
    bos_id = len(vocab)
    specials = [b"<|begin_of_text|>", b"<|end_of_text|>", b"<|start_header_id|>",
                b"<|end_header_id|>", b"<|eot_id|>"]
    vocab.extend(specials)
    scores.extend([0.0] * len(specials))
    eos_tokens = [bos_id + 1, bos_id + 4]  # end_of_text, eot_id
    if chat_template is None:
        chat_template = "{{<|start_header_id|>}}"  # auto-detects as llama3
    tok.write_tokenizer(path, vocab, scores, bos_id, True, eos_tokens, chat_template)


def make_tiny_llama(path: str, seed: int = 7, vocab_size: int = 512,
                    seq_len: int = 128, dim: int = 64) -> mf.LlmHeader:
    h = mf.LlmHeader(arch_type=mf.ARCH_LLAMA, dim=dim, hidden_dim=128, n_layers=2,
                     n_heads=4, n_kv_heads=2, head_dim=64, vocab_size=vocab_size,
                     seq_len=seq_len, rope_theta=10000, rope_type=mf.ROPE_LLAMA)
    h.finalize()
    mf.write_synthetic_model(path, h, seed=seed)
    return h


def make_tiny_qwen3(path: str, seed: int = 9, moe: bool = False,
                    dim: int = 64) -> mf.LlmHeader:
    if moe:
        h = mf.LlmHeader(arch_type=mf.ARCH_QWEN3_MOE, dim=dim, hidden_dim=96,
                         n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64,
                         n_experts=4, n_active_experts=2, moe_hidden_dim=64,
                         vocab_size=256, seq_len=64, rope_theta=10000,
                         norm_epsilon=1e-6)
    else:
        h = mf.LlmHeader(arch_type=mf.ARCH_QWEN3, dim=64, hidden_dim=96,
                         n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64,
                         vocab_size=256, seq_len=64, rope_theta=10000,
                         norm_epsilon=1e-6)
    h.finalize()
    mf.write_synthetic_model(path, h, seed=seed)
    return h
