"""True multi-process TP tests over gloo (world_size 2, one node).

This exercises the same torch.distributed code path the GPU uses with
RCCL (parallel/comm.py DistComm) — collectives, Q80 wire pack/unpack and
TP=2 vs TP=1 logits parity — without needing a GPU
(single-node run is the TP oracle)."""

import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from dllama_amd import model_file as mf
from dllama_amd.quants import F32
from dllama_amd.utils.testing import make_tiny_llama


def _worker(rank, world, path, port, out_q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["WORLD_SIZE"] = str(world)
        os.environ["RANK"] = str(rank)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from dllama_amd.models.config import ModelConfig
        from dllama_amd.models.cpu_model import CpuTransformer
        from dllama_amd.parallel.comm import DistComm

        m = mf.ModelFile(path, sync_type=F32)
        cfg = ModelConfig.from_header(m.header, world, rank)
        cfg.sync_type = F32
        model = CpuTransformer(m, cfg, DistComm())
        logits = model.forward(torch.tensor([3, 17, 101]), torch.arange(3))
        out_q.put((rank, logits.numpy()))
        dist.destroy_process_group()
    except Exception as e:  # noqa: BLE001
        out_q.put((rank, f"ERROR: {e!r}"))


@pytest.mark.timeout(180)
def test_tp2_gloo_matches_tp1(tmp_path):
    path = str(tmp_path / "tiny.m")
    make_tiny_llama(path, vocab_size=256)

    # single-rank reference
    from dllama_amd.models.config import ModelConfig
    from dllama_amd.models.cpu_model import CpuTransformer
    m = mf.ModelFile(path, sync_type=F32)
    cfg = ModelConfig.from_header(m.header)
    cfg.sync_type = F32
    ref = CpuTransformer(m, cfg).forward(torch.tensor([3, 17, 101]),
                                         torch.arange(3)).numpy()

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29571
    procs = [ctx.Process(target=_worker, args=(r, 2, path, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(2):
        rank, val = q.get(timeout=150)
        results[rank] = val
    for p in procs:
        p.join(timeout=60)
    for rank, val in results.items():
        assert not isinstance(val, str), val
        assert np.allclose(val, ref, atol=1e-4, rtol=1e-4), \
            f"rank {rank}: {np.abs(val - ref).max()}"


@pytest.mark.timeout(240)
def test_tp4_gloo_matches_tp1(tmp_path):
    """World=4 slicing (q/kv/ff/vocab all split 4-way) matches the
    single-rank oracle — exercises the deeper shard math the driver's
    round-end 8-GPU scaling run depends on (reference nn-core.cpp:211-285
    slicers at higher world sizes)."""
    path = str(tmp_path / "tiny4.m")
    h = mf.LlmHeader(arch_type=mf.ARCH_LLAMA, dim=64, hidden_dim=128,
                     n_layers=2, n_heads=4, n_kv_heads=4, head_dim=64,
                     vocab_size=256, seq_len=128, rope_theta=10000,
                     rope_type=mf.ROPE_LLAMA)
    h.finalize()
    mf.write_synthetic_model(path, h, seed=13)

    from dllama_amd.models.config import ModelConfig
    from dllama_amd.models.cpu_model import CpuTransformer
    m = mf.ModelFile(path, sync_type=F32)
    cfg = ModelConfig.from_header(m.header)
    cfg.sync_type = F32
    ref = CpuTransformer(m, cfg).forward(torch.tensor([3, 17, 101]),
                                         torch.arange(3)).numpy()

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 4, path, 29577, q))
             for r in range(4)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(4):
        rank, val = q.get(timeout=200)
        results[rank] = val
    for p in procs:
        p.join(timeout=60)
    for rank, val in results.items():
        assert not isinstance(val, str), val
        assert np.allclose(val, ref, atol=1e-4, rtol=1e-4), \
            f"rank {rank}: {np.abs(val - ref).max()}"


def _worker_moe(rank, world, path, port, out_q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                          WORLD_SIZE=str(world), RANK=str(rank))
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from dllama_amd.models.config import ModelConfig
        from dllama_amd.models.cpu_model import CpuTransformer
        from dllama_amd.parallel.comm import DistComm
        m = mf.ModelFile(path, sync_type=F32)
        cfg = ModelConfig.from_header(m.header, world, rank)
        cfg.sync_type = F32
        model = CpuTransformer(m, cfg, DistComm())
        logits = model.forward(torch.tensor([1, 5, 9]), torch.arange(3))
        out_q.put((rank, logits.numpy()))
        dist.destroy_process_group()
    except Exception as e:  # noqa: BLE001
        out_q.put((rank, f"ERROR: {e!r}"))


@pytest.mark.timeout(180)
def test_tp2_gloo_moe(tmp_path):
    """Qwen3-MoE TP=2 over gloo matches TP=1 (expert slices + redundant
    gate, reference SURVEY §2.2 EP row)."""
    from dllama_amd.utils.testing import make_tiny_qwen3
    path = str(tmp_path / "moe.m")
    make_tiny_qwen3(path, moe=True)
    from dllama_amd.models.config import ModelConfig
    from dllama_amd.models.cpu_model import CpuTransformer
    m = mf.ModelFile(path, sync_type=F32)
    cfg = ModelConfig.from_header(m.header)
    cfg.sync_type = F32
    ref = CpuTransformer(m, cfg).forward(torch.tensor([1, 5, 9]),
                                         torch.arange(3)).numpy()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_moe, args=(r, 2, path, 29573, q))
             for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(2):
        rank, val = q.get(timeout=150)
        results[rank] = val
    for p in procs:
        p.join(timeout=60)
    for rank, val in results.items():
        assert not isinstance(val, str), val
        assert np.allclose(val, ref, atol=1e-4, rtol=1e-4)


@pytest.mark.timeout(240)
def test_bench_driver_contract_tp2_cpu():
    """Launch bench.py EXACTLY the way the round-end driver does
    (torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py
    --gpus N) using the hidden --device cpu smoke mode: validates torchrun
    env parsing, init_dist_comm, Q80 wire sync over collectives,
    max-over-ranks timing and the rank-0 JSON line without a GPU."""
    import json
    import subprocess
    import sys as _sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(
        [_sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29583", "bench.py", "--gpus", "2",
         "--device", "cpu", "--steps", "4", "--warmup", "1",
         "--prefill", "8"],
        cwd=repo, capture_output=True, text=True, timeout=220)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, out.stdout  # exactly ONE JSON line (rank 0 only)
    j = json.loads(line[0])
    assert j["n_gpus"] == 2 and j["steps"] == 4
    assert j["config"]["parallelism"] == "tp2"
    assert j["value"] > 0 and j["ms_per_step"] > 0


@pytest.mark.timeout(120)
def test_bench_dump_outputs_cpu(tmp_path):
    """bench.py --dump-outputs writes the last timed step's logits and
    greedy token as float .npy files, identical from run to run with the
    same arguments and different once --steps changes the last step; the
    result line keeps its fields and --full is accepted."""
    import json
    import subprocess
    import sys as _sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(name, steps, *extra):
        d = tmp_path / name
        out = subprocess.run(
            [_sys.executable, "bench.py", "--gpus", "1", "--device", "cpu",
             "--steps", str(steps), "--warmup", "1", "--prefill", "8",
             "--dump-outputs", str(d), *extra],
            cwd=repo, capture_output=True, text=True, timeout=100)
        assert out.returncode == 0, out.stderr[-2000:]
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(line) == 1, out.stdout
        j = json.loads(line[0])
        assert j["steps"] == steps and j["ms_per_step"] > 0
        for key in ("metric", "value", "unit", "higher_is_better", "dtype"):
            assert key in j
        assert sorted(os.listdir(d)) == ["logits.npy", "next_token.npy"]
        return {n: np.load(d / f"{n}.npy") for n in ("logits", "next_token")}

    a, b, c = run("a", 3), run("b", 3, "--full"), run("c", 4)
    assert a["logits"].dtype == np.float32 and a["logits"].shape == (256,)
    assert a["next_token"].dtype == np.float64
    assert np.isfinite(a["logits"]).all()
    assert int(a["next_token"][0]) == int(a["logits"].argmax())
    for n in a:
        assert np.array_equal(a[n], b[n]), n
    # one more step moves the decode one position on: other logits
    assert not np.array_equal(a["logits"], c["logits"])


@pytest.mark.timeout(120)
def test_bench_uses_built_extension_without_jit_load():
    """bench.py imports the built extension straight from the tree: torch's
    JIT load(), which needs to write a lock file into the build directory,
    must not run when the library is already there."""
    import subprocess
    import sys as _sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from dllama_amd.ops import hip_ops
    hip_ops()  # make sure it is built (the suite runs after the build)
    code = (
        "import os, torch.utils.cpp_extension as ce\n"
        "def boom(*a, **k): raise AssertionError('JIT load() was called')\n"
        "ce.load = boom\n"
        "import bench\n"
        "bench._use_built_extension()\n"
        "from dllama_amd.ops import hip_ops\n"
        "m = hip_ops()\n"
        "assert os.path.dirname(m.__file__).endswith(os.path.join('ops', '_build'))\n"
        "print('native', m.__file__)\n")
    out = subprocess.run([_sys.executable, "-c", code], cwd=repo,
                         capture_output=True, text=True, timeout=100)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "native" in out.stdout


def _api_tp_worker(rank, world, mp_path, tp_path, port, out_q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["WORLD_SIZE"] = str(world)
        os.environ["RANK"] = str(rank)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from dllama_amd.apps.api import ApiState
        from dllama_amd.apps.main import build_parser
        from dllama_amd.parallel.lockstep import RootModel, follower_loop
        args = build_parser().parse_args(
            ["inference", "--model", mp_path, "--tokenizer", tp_path,
             "--gpu-index", "-1", "--temperature", "0", "--seed", "1",
             "--buffer-float-type", "f32"])
        state = ApiState(args)
        body = {"messages": [{"role": "user", "content": "abc"}],
                "max_tokens": 6, "temperature": 0}
        if rank == 0:
            state.engine.model = RootModel(state.engine.model, state.comm)
            text, _, n_gen = state.complete(body, lambda d: None)
            state.engine.model.stop_followers()
            out_q.put((0, (text, n_gen)))
        else:
            n = follower_loop(state.engine.model, state.comm)
            out_q.put((1, n))
        dist.destroy_process_group()
    except Exception as e:  # noqa: BLE001
        out_q.put((rank, f"ERROR: {e!r}"))


@pytest.mark.timeout(240)
def test_api_tp2_root_follower(tmp_path):
    """dllama-api under TP: rank 0 serves + samples, rank 1 replays control
    packets (reference root/worker split, app.cpp:168-230). The TP=2
    completion must equal a single-rank completion of the same request."""
    from dllama_amd.utils.testing import make_byte_tokenizer
    mp_path = str(tmp_path / "tiny.m")
    tp_path = str(tmp_path / "tiny.t")
    make_byte_tokenizer(tp_path)
    from dllama_amd.tokenizer import Tokenizer
    vocab = Tokenizer(tp_path).vocab_size
    make_tiny_llama(mp_path, vocab_size=vocab + (32 - vocab % 32) % 32)

    # single-rank reference completion
    from dllama_amd.apps.api import ApiState
    from dllama_amd.apps.main import build_parser
    os.environ.pop("WORLD_SIZE", None)
    args = build_parser().parse_args(
        ["inference", "--model", mp_path, "--tokenizer", tp_path,
         "--gpu-index", "-1", "--temperature", "0", "--seed", "1",
         "--buffer-float-type", "f32"])
    ref_state = ApiState(args)
    body = {"messages": [{"role": "user", "content": "abc"}],
            "max_tokens": 6, "temperature": 0}
    want_text, _, want_n = ref_state.complete(body, lambda d: None)

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_api_tp_worker,
                         args=(r, 2, mp_path, tp_path, 29573, q))
             for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=200) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
    assert not isinstance(res[0], str), res[0]
    assert not isinstance(res[1], str), res[1]
    text, n_gen = res[0]
    assert (text, n_gen) == (want_text, want_n)
    assert res[1] >= n_gen  # follower replayed prefill + decode forwards
