#!/usr/bin/env python3
"""Cross-validation against the reference C++ implementation.

Builds b4rtaz/distributed-llama's `dllama` from /root/reference (pure C++,
CPU), writes a tiny synthetic model + ASCII-only tokenizer with THIS
framework's .m/.t writers, then greedy-decodes the same prompt with both
runtimes and compares the generated text exactly.

This proves end-to-end: file-format byte compatibility, weight-walk order,
Q40/Q80 quantization parity, and model-math parity (same argmax trajectory).
"""

import os
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from dllama_amd import model_file as mf
from dllama_amd import tokenizer as tk

# checkout of b4rtaz/distributed-llama to build the reference binary from
REF_SRC = os.environ.get("DLLAMA_REFERENCE_SRC", "")

# the reference's recorded outputs for CASES/CHAT_CASE below, with the
# sha256 of the exact .m/.t files it consumed (tests replay against these
# without the reference; `--record` regenerates the file)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                      "tests", "golden", "reference_parity.json")

# per-arch vocab picks a trajectory with decisive greedy margins (a near-tie
# anywhere flips between the reference's int8 path and the f32 oracle); chat
# needs the filler-free 101 vocab (duplicate '~' embeddings = near-tie runs
# on long decodes)
CASES = [{"arch": "llama", "vocab_size": 101},
         {"arch": "qwen3", "vocab_size": 128},
         {"arch": "qwen3_moe", "vocab_size": 128}]
PROMPT, STEPS = "hello world, this is", 48
CHAT_CASE = {"arch": "llama", "vocab_size": 101, "system": "keep it short",
             "users": ["hello ab", "more cd"]}


def file_sha256(path: str) -> str:
    import hashlib
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def record(workdir: str, binary: str) -> dict:
    """Run the reference on every case and return the golden record."""
    gold = {"prompt": PROMPT, "steps": STEPS, "generate": [], "chat": None}
    for case in CASES:
        model, tok = make_ascii_assets(workdir, **case)
        gold["generate"].append(dict(
            case, model_sha256=file_sha256(model),
            tokenizer_sha256=file_sha256(tok),
            text=run_reference(binary, model, tok, PROMPT, STEPS)))
    c = CHAT_CASE
    model, tok = make_ascii_assets(workdir, vocab_size=c["vocab_size"],
                                   arch=c["arch"])
    gold["chat"] = dict(
        c, model_sha256=file_sha256(model), tokenizer_sha256=file_sha256(tok),
        turns=run_reference_chat(binary, model, tok, c["system"], c["users"]))
    return gold


def build_reference(workdir: str) -> str:
    # a prebuilt binary (tools/_refbin/dllama, gitignored) lets the harness
    # run on GPU boxes where /root/reference is not present
    prebuilt = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                            "_refbin", "dllama")
    if not os.path.isdir(REF_SRC) and os.path.exists(prebuilt):
        return prebuilt
    ref = os.path.join(workdir, "refbuild")
    if not os.path.exists(ref) and not os.path.isdir(REF_SRC):
        raise SystemExit("set DLLAMA_REFERENCE_SRC to a checkout of "
                         "b4rtaz/distributed-llama")
    if not os.path.exists(ref):
        shutil.copytree(REF_SRC, ref)
    binary = os.path.join(ref, "dllama")
    if not os.path.exists(binary):
        subprocess.run(["make", "dllama"], cwd=ref, check=True,
                       capture_output=True)
    return binary


def make_ascii_assets(workdir: str, vocab_size: int = 101, arch: str = "llama"):
    """Tokenizer whose every regular token is printable ASCII -> decode is
    lossless text on both sides. No duplicate filler tokens: the structured
    model's greedy walk visits consecutive ids, and duplicate-embedding
    runs have near-tie margins that flip between the reference's int8 path
    and the f32 oracle on long chat decodes."""
    # newline included: the llama3 chat template emits "\n\n"
    printable = [b"\n"] + [chr(c).encode() for c in range(0x20, 0x7F)]
    vocab = list(printable) + [b"~"] * (vocab_size - 5 - len(printable))
    scores = [0.0] * len(vocab)
    bos_id = len(vocab)
    # llama3-named specials so the chat template's literal special-token
    # strings are encodable (chat-mode parity needs this)
    vocab += [b"<|begin_of_text|>", b"<|end_of_text|>", b"<|start_header_id|>",
              b"<|end_header_id|>", b"<|eot_id|>"]
    scores += [0.0] * 5
    tok_path = os.path.join(workdir, "parity.t")
    tk.write_tokenizer(tok_path, vocab, scores, bos_id, True,
                       [bos_id + 1, bos_id + 4],  # end_of_text, eot_id
                       "{{<|start_header_id|>}}")

    if arch == "qwen3_moe":
        h = mf.LlmHeader(arch_type=mf.ARCH_QWEN3_MOE, dim=64, hidden_dim=128,
                         n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64,
                         n_experts=4, n_active_experts=2, moe_hidden_dim=64,
                         vocab_size=vocab_size, seq_len=256, rope_theta=10000,
                         norm_epsilon=1e-6)
    elif arch == "qwen3":
        h = mf.LlmHeader(arch_type=mf.ARCH_QWEN3, dim=64, hidden_dim=128,
                         n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64,
                         vocab_size=vocab_size, seq_len=256, rope_theta=10000,
                         norm_epsilon=1e-6)
    else:
        h = mf.LlmHeader(arch_type=mf.ARCH_LLAMA, dim=64, hidden_dim=128,
                         n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64,
                         vocab_size=vocab_size, seq_len=256, rope_theta=10000,
                         rope_type=mf.ROPE_LLAMA)
    h.finalize()
    model_path = os.path.join(workdir, f"parity_{arch}.m")
    write_structured_model(model_path, h)
    return model_path, tok_path


def write_structured_model(path: str, h: mf.LlmHeader, seed: int = 11) -> None:
    """Random model EXCEPT wcls[i] = embedding[i-1]: logits argmax is
    'input token + 1' with decisive margins, so greedy trajectories are
    robust to rounding-mode differences between runtimes (a fully random
    model has near-flat logits and argmax ties flip on 1-ulp noise)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((h.vocab_size, h.dim)).astype(np.float32) * 0.03
    with open(path, "wb") as f:
        mf.write_header(f, h)
    hdr = mf.read_header(path)
    with open(path, "ab") as f:
        for e in mf.tensor_walk(hdr):
            if e.name == "embedding":
                x = emb
            elif e.name == "final_matmul_logits":
                x = np.roll(emb, 1, axis=0)  # wcls[i] = emb[i-1]
            elif e.name in ("block_norm_0", "block_norm_1", "final_norm"):
                x = np.ones(int(np.prod(e.shape)), dtype=np.float32)
            else:
                x = rng.standard_normal(int(np.prod(e.shape))).astype(np.float32) * 0.03
            mf.write_tensor(f, x, e.float_type)


def run_reference(binary, model, tok, prompt, steps) -> str:
    out = subprocess.run(
        [binary, "inference", "--model", model, "--tokenizer", tok,
         "--prompt", prompt, "--steps", str(steps), "--temperature", "0",
         "--nthreads", "2", "--buffer-float-type", "q80",
         "--max-seq-len", "256"],
        capture_output=True, text=True, timeout=300, check=True)
    pieces = []
    for line in out.stdout.splitlines():
        if line.startswith("🔶"):
            pieces.append(line.rsplit("| ", 1)[1] if "| " in line else "")
    return "".join(pieces)


def run_ours(model, tok_path, prompt, steps) -> str:
    """Greedy-decode with the REFERENCE's prompt handoff emulated.

    The reference inference loop has an off-by-one (dllama.cpp:56 reads
    `inputTokens[pos + 1]` after `pos += batchSize`), so its decode starts
    from a zero token at position n-1 instead of the last prompt token.
    To compare trajectories we reproduce exactly that: prefill
    tokens[:-1] + [0], then sample steps-n+1 tokens.
    (dllama_amd's own engine uses the correct handoff.)"""
    from dllama_amd.engine import InferenceEngine
    from dllama_amd.models.config import ModelConfig
    from dllama_amd.models.cpu_model import CpuTransformer
    from dllama_amd.tokenizer import Sampler, Tokenizer
    m = mf.ModelFile(model, max_seq_len=256)
    tok = Tokenizer(tok_path)
    cfg = ModelConfig.from_header(m.header)
    if USE_HIP:
        from dllama_amd.models.hip_model import HipTransformer
        net = HipTransformer.from_file(m, cfg)
    else:
        net = CpuTransformer(m, cfg)
    eng = InferenceEngine(net, tok,
                          Sampler(m.header.vocab_size, 0.0, 0.9, 1))
    tokens = tok.encode(prompt)
    emulated = tokens[:-1] + [0]
    out, _ = eng.generate(emulated, steps - len(tokens) + 1)
    tok.reset_decoder()
    return "".join(p for p in (tok.decode(t) for t in out) if p)


def run_reference_chat(binary, model, tok, sys_prompt, users):
    """Scripted multi-turn chat against the reference binary; returns the
    assistant text of each turn. The reference spins on stdin EOF, so a
    timeout + kill is part of the protocol (partial output is kept)."""
    stdin = sys_prompt + "\n" + "\n".join(users) + "\n"
    # No stdbuf here: its LD_PRELOAD shifts the heap layout and the
    # reference chat's handoff token (`inputTokens[i + 1]` one past the
    # prompt, dllama.cpp:223) is UNINITIALIZED memory — zero in the plain
    # environment (what this harness locks in), garbage -> segfault under
    # stdbuf. Pipe stdout is fully buffered, so completion cannot be
    # detected incrementally; keep stdin OPEN after the scripted turns (on
    # EOF readStdin re-prompts in a tight loop, GBs of spam; blocked in
    # fgets it is quiet), give the turns a fixed window, then kill and
    # collect the buffered output.
    p = subprocess.Popen(
        [binary, "chat", "--model", model, "--tokenizer", tok,
         "--temperature", "0", "--nthreads", "2", "--buffer-float-type",
         "q80", "--max-seq-len", "256"],
        stdin=subprocess.PIPE, stdout=subprocess.PIPE,
        stderr=subprocess.DEVNULL)
    p.stdin.write(stdin.encode())
    p.stdin.flush()
    try:
        p.wait(timeout=30)
    except subprocess.TimeoutExpired:
        p.kill()
    p.wait()
    out = p.stdout.read().decode("utf-8", "replace")
    p.stdout.close()
    p.stdin.close()
    turns = []
    for part in out.split("🤖 Assistant\n")[1:]:
        for stop in ("\n👱 User", "👱 User", "(end of context)"):
            i = part.find(stop)
            if i >= 0:
                part = part[:i]
        turns.append(part)
    return turns


def run_ours_chat(model, tok_path, sys_prompt, users):
    """Multi-turn chat with THIS framework's template generator, tokenizer,
    EOS detector and CPU model — reproducing the reference chat loop's
    prompt handoff (dllama.cpp:223: after the prefill loop the next decode
    token is read one past the encoded prompt, i.e. a zero) so trajectories
    are comparable. Returns per-turn assistant text."""
    import torch
    from dllama_amd.models.config import ModelConfig
    from dllama_amd.models.cpu_model import CpuTransformer
    from dllama_amd.tokenizer import (ChatItem, ChatTemplateGenerator,
                                      EosDetector, Tokenizer, chat_stops,
                                      EOS, MAYBE_EOS, TEMPLATE_UNKNOWN)
    m = mf.ModelFile(model, max_seq_len=256)
    tok = Tokenizer(tok_path)
    net = CpuTransformer(m, ModelConfig.from_header(m.header))
    seq_len = m.header.seq_len
    stops = chat_stops(tok)
    max_stop = max(len(s) for s in stops)
    gen = ChatTemplateGenerator(TEMPLATE_UNKNOWN, tok.chat_template,
                                stops[0])
    pos = 0
    turns = []
    for i, user in enumerate(users):
        items = []
        if i == 0 and sys_prompt:
            items.append(ChatItem("system", sys_prompt))
        items.append(ChatItem("user", user))
        text = gen.generate(items, True).content
        tokens = tok.encode(text, is_start=(pos == 0))
        if pos + len(tokens) - 1 >= seq_len:
            break
        # prefill tokens[:-1]; the reference's decode handoff token is the
        # uninitialized slot one past the prompt (zero in practice)
        n_feed = len(tokens) - 1
        for j in range(0, n_feed, 32):
            chunk = tokens[j: min(j + 32, n_feed)]
            net.forward(torch.tensor(chunk),
                        torch.arange(pos, pos + len(chunk)))
            pos += len(chunk)
        token = 0
        tok.reset_decoder()
        det = EosDetector(tok.eos_token_ids, stops, max_stop, max_stop)
        out = []
        while pos < seq_len:
            logits = net.forward(torch.tensor([token]), torch.tensor([pos]))
            token = int(torch.argmax(logits[0]))
            pos += 1
            kind = det.append(token, tok.decode(token))
            if kind != MAYBE_EOS:
                delta = det.get_delta()
                if delta:
                    out.append(delta)
                det.reset()
            if kind == EOS:
                break
        turns.append("".join(out))
    return turns


USE_HIP = "--hip" in sys.argv  # greedy-compare the GPU path itself


def main():
    argv = [a for a in sys.argv[1:] if a not in ("--hip", "--record")]
    workdir = argv[0] if argv else tempfile.mkdtemp(prefix="parity")
    os.makedirs(workdir, exist_ok=True)
    binary = build_reference(workdir)
    if "--record" in sys.argv:
        import json
        with open(GOLDEN, "w") as f:
            json.dump(record(workdir, binary), f, indent=1, ensure_ascii=True)
            f.write("\n")
        print(f"recorded reference outputs -> {os.path.normpath(GOLDEN)}")
        return 0
    rc = 0
    for arch in ("llama", "qwen3", "qwen3_moe"):
        # per-arch vocab picks a trajectory with decisive greedy margins
        # (a near-tie anywhere flips between the reference's int8 path and
        # the f32 oracle); chat needs the filler-free 101 vocab (duplicate
        # '~' embeddings = near-tie runs on long decodes)
        model, tok = make_ascii_assets(
            workdir, vocab_size=101 if arch == "llama" else 128, arch=arch)
        prompt = "hello world, this is"
        steps = 48
        ref_text = run_reference(binary, model, tok, prompt, steps)
        our_text = run_ours(model, tok, prompt, steps)
        print(f"[{arch}] reference: {ref_text!r}")
        print(f"[{arch}] dllama_amd:{our_text!r}")
        if ref_text == our_text:
            print(f"✅ [{arch}] PARITY: {steps} greedy tokens identical "
                  "(format + quantization + model math)")
        else:
            n = sum(1 for a, b in zip(ref_text, our_text) if a == b)
            print(f"❌ [{arch}] MISMATCH after {n} matching chars")
            rc = 1

    if USE_HIP:
        return rc  # chat-mode parity is the CPU harness's job
    # chat-mode parity (llama): template generation, multi-turn KV
    # continuity, EOS detection — vs the reference's interactive loop
    model, tok = make_ascii_assets(workdir, arch="llama")
    sys_prompt, users = "keep it short", ["hello ab", "more cd"]
    ref_turns = run_reference_chat(binary, model, tok, sys_prompt, users)
    our_turns = run_ours_chat(model, tok, sys_prompt, users)
    print(f"[chat] reference turns: {[t[:40] for t in ref_turns]!r}")
    print(f"[chat] dllama_amd turns:{[t[:40] for t in our_turns]!r}")
    if ref_turns and ref_turns == our_turns:
        print(f"✅ [chat] PARITY: {len(ref_turns)} multi-turn assistant "
              "replies identical (template + KV continuity + EOS)")
    else:
        print("❌ [chat] MISMATCH")
        rc = 1
    return rc


if __name__ == "__main__":
    sys.exit(main())
