"""Greedy-trajectory parity against the reference C++ runtime.

The reference's outputs are recorded in tests/golden/reference_parity.json
(`python tools/reference_parity.py --record` regenerates it from a build of
the reference), together with the sha256 of the exact model and tokenizer
files it read. The test rewrites those files with this framework's
writers, requires them byte-identical to what the reference consumed, and
compares its own decode with the recorded text. See
tools/reference_parity.py and profiles/reference_parity.md."""

import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), "tools"))


@pytest.mark.timeout(600)
def test_greedy_parity_with_reference(tmp_path):
    import reference_parity as rp
    with open(rp.GOLDEN) as f:
        gold = json.load(f)
    workdir = str(tmp_path)
    prompt, steps = gold["prompt"], gold["steps"]
    assert (prompt, steps) == (rp.PROMPT, rp.STEPS)
    assert [g["arch"] for g in gold["generate"]] == ["llama", "qwen3",
                                                     "qwen3_moe"]
    for g in gold["generate"]:
        arch = g["arch"]
        model, tok = rp.make_ascii_assets(
            workdir, vocab_size=g["vocab_size"], arch=arch)
        # the files the recorded run read, byte for byte
        assert rp.file_sha256(model) == g["model_sha256"], arch
        assert rp.file_sha256(tok) == g["tokenizer_sha256"], arch
        ref = g["text"]
        assert len(ref) > 0
        ours = rp.run_ours(model, tok, prompt, steps)
        assert ref == ours, f"{arch}: {ref!r} != {ours!r}"

    # multi-turn chat parity (template generation, KV continuity across
    # turns, EOS detection) against the reference's interactive loop
    c = gold["chat"]
    model, tok = rp.make_ascii_assets(workdir, vocab_size=c["vocab_size"],
                                      arch=c["arch"])
    assert rp.file_sha256(model) == c["model_sha256"]
    assert rp.file_sha256(tok) == c["tokenizer_sha256"]
    assert (c["system"], c["users"]) == ("keep it short",
                                         ["hello ab", "more cd"])
    ref_turns = c["turns"]
    our_turns = rp.run_ours_chat(model, tok, c["system"], c["users"])
    assert len(ref_turns) == 2, ref_turns
    assert ref_turns == our_turns, (ref_turns, our_turns)
