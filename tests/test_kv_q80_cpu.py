"""The Q80 KV cache on the CPU: the stored-block round trip of
ops/reference.py, CpuTransformer(kv_dtype="q80") as the oracle of the HIP
backend's Q80 cache (against the f32-cache oracle, and paged against unpaged),
and the --kv-dtype option of the apps."""

import re

import numpy as np
import pytest
import torch

from dllama_amd import model_file as mf
from dllama_amd import quants
from dllama_amd.models.config import ModelConfig
from dllama_amd.models.cpu_model import CpuTransformer
from dllama_amd.ops import reference as R
from dllama_amd.utils.testing import (make_byte_tokenizer, make_tiny_llama,
                                      make_tiny_qwen3)

from test_rows_model import SCHEDULE, SLOT_OF, TOKENS, _drive

P = 4
# slot -> pool pages, scrambled (slots as SLOT_OF: the 9-, 5- and 13-token
# sequences live in slots 2, 0 and 3)
PAGES_OF = {2: [11, 3, 7], 0: [5, 14], 3: [2, 9, 0, 13]}
KV_PAGES = 16


def test_roundtrip_f16_equals_quants():
    """The torch helper and the numpy block codec: same codes, same f16
    scale, same product."""
    g = torch.Generator().manual_seed(80)
    x = torch.randn(7, 256, generator=g) * 3.0
    x[2, 32:64] = 0.0  # an all-zero block: code 0, scale 0
    x[5, 0] = 1e-6     # and a block whose scale is an f16 subnormal
    x[5, 1:32] = 0.0
    want = torch.from_numpy(quants.q80_roundtrip(x.numpy()))
    got = R.q80_roundtrip_f16(x)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    q, s = R.q80_quantize_f16(x)
    assert q.dtype == torch.int8 and s.dtype == torch.float16
    assert s.shape == (7, 8)
    blocks = quants.quantize_q80(x.numpy()).reshape(7, 8, 34)
    assert np.array_equal(blocks[:, :, 2:].view(np.int8).reshape(7, 256),
                          q.numpy())
    assert np.array_equal(blocks[:, :, :2].copy().view(np.float16)
                          .reshape(7, 8), s.numpy())
    # not the activation cast, which keeps d in f32
    assert not torch.equal(got, R.q80_roundtrip(x))


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("kvq80cpu")
    out = {}
    for arch in TOKENS:
        p = str(d / f"{arch}.m")
        if arch == "llama":
            make_tiny_llama(p, vocab_size=256)
        else:
            make_tiny_qwen3(p, moe=arch == "qwen3moe")
        m = mf.ModelFile(p)
        out[arch] = (m, ModelConfig.from_header(m.header))
    return out


@pytest.mark.parametrize("arch", list(TOKENS))
def test_cpu_q80_oracle_close_to_f32(models, arch):
    """The round trip is taken (the logits differ), costs less than 1% of
    the row maximum, and moves no argmax."""
    m, cfg = models[arch]
    for s, toks in enumerate(TOKENS[arch]):
        t, pos = torch.tensor(toks), torch.arange(len(toks))
        f32 = CpuTransformer(m, cfg).forward(t, pos)
        same = CpuTransformer(m, cfg, kv_dtype="f16").forward(t, pos)
        assert torch.equal(same, f32)  # any other value: the f32 cache
        q80 = CpuTransformer(m, cfg, kv_dtype="q80").forward(t, pos)
        assert not torch.equal(q80, f32)
        rel = ((q80 - f32).abs().max(dim=1).values
               / f32.abs().max(dim=1).values).max().item()
        print(f"{arch} seq {s}: q80 vs f32 cache rel diff {rel:.5f}")
        assert rel < 0.01, (arch, s, rel)
        assert torch.equal(q80.argmax(-1), f32.argmax(-1)), (arch, s)


@pytest.mark.parametrize("arch", list(TOKENS))
def test_cpu_q80_paged_equals_unpaged(models, arch):
    m, cfg = models[arch]
    want = _drive(CpuTransformer(m, cfg, n_slots=4, kv_dtype="q80"), arch)
    paged = CpuTransformer(m, cfg, n_slots=4, kv_pages=KV_PAGES, page_size=P,
                           kv_dtype="q80")
    for slot, pages in PAGES_OF.items():
        paged.set_slot_pages(slot, pages)
    got = _drive(paged, arch)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    # and the row schedule is the sequences alone
    for s, toks in enumerate(TOKENS[arch]):
        alone = CpuTransformer(m, cfg, kv_dtype="q80").forward(
            torch.tensor(toks), torch.arange(len(toks)))
        assert torch.allclose(want[s], alone, rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------ the apps

@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    d = tmp_path_factory.mktemp("kvq80app")
    mp, tp = str(d / "tiny.m"), str(d / "tiny.t")
    make_byte_tokenizer(tp)
    from dllama_amd.tokenizer import Tokenizer
    vocab = Tokenizer(tp).vocab_size
    make_tiny_llama(mp, vocab_size=vocab + (32 - vocab % 32) % 32)
    return mp, tp


def _disk_line(out):
    return next(l for l in out.splitlines() if l.startswith("📀"))


def test_cli_kv_dtype(assets, capsys):
    from dllama_amd.apps.main import build_parser, main
    mp, tp = assets
    assert build_parser().parse_args(["inference"]).kv_dtype is None
    common = ["inference", "--model", mp, "--tokenizer", tp, "--steps", "4",
              "--temperature", "0", "--gpu-index", "-1", "--prompt", "abc"]
    assert main(common) == 0
    plain = _disk_line(capsys.readouterr().out)
    assert "bytes" not in plain and "q80" not in plain
    figures = {}
    for dt in ("f32", "q80"):
        assert main([*common, "--kv-dtype", dt]) == 0
        line = _disk_line(capsys.readouterr().out)
        gb, name, nbytes = re.search(
            r"KV cache/rank: ([\d.]+) GB \((\w+), (\d+) bytes, seq", line
        ).groups()
        assert name == dt
        figures[dt] = (gb, int(nbytes))
    # the default line counts f32: the same figure as --kv-dtype f32 ...
    assert re.search(r"KV cache/rank: ([\d.]+) GB \(seq", plain).group(1) \
        == figures["f32"][0]
    # ... of which q80 is (1 + 2/32) / 4 = 0.53125 / 2
    assert figures["q80"][1] * 2 == figures["f32"][1] * 0.53125


def test_cli_refuses_unknown_kv_dtype(assets, capsys):
    from dllama_amd.apps.main import main
    mp, tp = assets
    with pytest.raises(SystemExit):
        main(["inference", "--model", mp, "--tokenizer", tp, "--gpu-index",
              "-1", "--prompt", "abc", "--kv-dtype", "q4"])
    assert "--kv-dtype" in capsys.readouterr().err
    from dllama_amd.apps import api as api_mod
    with pytest.raises(SystemExit):
        api_mod.main(["--model", mp, "--tokenizer", tp, "--gpu-index", "-1",
                      "--kv-dtype", "q4"])
