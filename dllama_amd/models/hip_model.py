"""MI355X transformer: device-resident Q40 weights + hand-written HIP kernels.

Architecture (MI355X-first):
  - weights repacked at load into the GEMV device layout (nibble plane
    uint8 [d, n/2] + f16 scale plane [d, n/32]) — the .m block stream is
    only a wire format;
  - all activations live in preallocated device buffers sized for the max
    batch, so the whole decode step is hipGraph-capturable (reference
    replays recorded Vulkan command buffers the same way,
    nn-vulkan.cpp:1065-1118);
  - the position is a device int32 tensor read by rope/kv/attention kernels
    — no host round-trip per token;
  - TP sync = on-device Q80 pack -> RCCL all-gather -> merge-add kernel
    (reference SYNC_NODE_SLICES + OP_MERGE_ADD) or plain f32 all-reduce
    (sync_type f32).

Three launch schedules share one set of stages (the `_`-prefixed methods
under "stages": each kernel call site with its argument plumbing exists
once): `_forward_explicit` (explicit norm_quant per matmul; any batch),
`_forward_dense_deferred` (B=1 decode, quantization deferred into the
producers' epilogues) and `_forward_prefill_bf16` (library bf16 GEMMs, an
A/B baseline). `forward_buffers` picks among them for a single-sequence
step. tests/test_launch_trace.py pins the resulting launch sequences.

Rope, KV write and attention reach a row's position and cache rows through
a `KVAddr`. The single-sequence value says "row b is position pos+b of slot
0". A row step (`forward_rows`, docs/DESIGN.md §8) runs the explicit-norm
schedule with the row-table value instead: the KV cache holds `n_slots`
sequences and a per-row {cache row base, position} table places each row,
so one step carries rows of several sequences. With `kv_pages > 0` the
value also names a device page table: the cache is a pool of pages and each
slot reaches its rows through it. With the default of one slot nothing of
this is allocated or launched.

Which steps replay a captured hipGraph is asked of one store, `self.graphs`
(models/graphs.py); the step that first needs a graph captures it.
"""

from __future__ import annotations

import os
import sys
from functools import partial

import numpy as np
import torch

from ..model_file import HIDDEN_ACT_GELU, ModelFile, ROPE_FALCON
from ..ops import hip_ops
from ..ops import reference as R
from ..ops.sampler import DeviceSampler
from ..parallel.comm import Comm, SingleComm
from ..quants import Q80, q40_to_planes
from .config import ModelConfig
from .graphs import StepGraphs, capture_hip_graph

QB = 32
# logprob_rows results per row: f32 {lse, logprob, top-20 logprobs} and i32
# top-20 ids; with the row's {token, status} that is LP_WORDS int64 words
LP_MAXK = R.LOGPROB_MAXK
LP_F32 = 2 + LP_MAXK
LP_WORDS = 2 + LP_F32 // 2 + LP_MAXK // 2


class Linear:
    """A Q40 linear layer shard on device: y = W x."""

    def __init__(self, qs: torch.Tensor, scales: torch.Tensor):
        self.qs = qs          # uint8 [d, n/2] (or [E, d, n/2])
        self.scales = scales  # f16  [d, n/32] (or [E, d, n/32])
        self.d = qs.shape[-2]
        self.n = qs.shape[-1] * 2

    @classmethod
    def from_blocks(cls, raw: np.ndarray, d: int, n: int, device) -> "Linear":
        qs, sc = q40_to_planes(raw, d, n)
        return cls(torch.from_numpy(qs).to(device),
                   torch.from_numpy(sc).to(device))

    @classmethod
    def synthetic(cls, d: int, n: int, device, gen: torch.Generator,
                  scale: float = 0.02, experts: int | None = None) -> "Linear":
        lead = () if experts is None else (experts,)
        qs = torch.randint(0, 256, (*lead, d, n // 2), dtype=torch.uint8,
                           device=device, generator=gen)
        sc = (torch.rand((*lead, d, n // QB), device=device, generator=gen)
              * scale / 8)
        return cls(qs, sc.to(torch.float16))

    @classmethod
    def cat(cls, *parts: "Linear") -> "Linear":
        """Fuse along the output rows: one GEMV launch, one pass over x."""
        return cls(torch.cat([p.qs for p in parts]),
                   torch.cat([p.scales for p in parts]))

    @classmethod
    def stack(cls, parts: list) -> "Linear":
        """Experts along a new leading dimension (grouped GEMV layout)."""
        return cls(torch.stack([p.qs for p in parts]),
                   torch.stack([p.scales for p in parts]))


class QuantBuf:
    """Q80 activation triple for a [rows, n] buffer."""

    def __init__(self, rows: int, n: int, device):
        self.n = n
        self.q = torch.zeros(rows, n, dtype=torch.int8, device=device)
        self.s = torch.zeros(rows, n // QB, dtype=torch.float32, device=device)
        self.bs = torch.zeros(rows, n // QB, dtype=torch.float32, device=device)

    def triple(self, rows: int | None = None):
        """(q, s, bs): the whole buffers, or their first `rows` rows."""
        if rows is None:
            return self.q, self.s, self.bs
        return self.q[:rows], self.s[:rows], self.bs[:rows]


def _pow2_batch(b: int) -> int:
    nb = 1
    while nb < b:
        nb *= 2
    return nb


class KVAddr:
    """How the positional kernels (rope, KV write, attention) find batch row
    b's position and its sequence's cache rows. Three values exist:

      KVAddr("", pos, attn_scratch=(attn_counter,))
          one sequence: row b is position pos[0]+b of slot 0;
      KVAddr("_rows", rows)
          the row table {cache row base, position} per row;
      KVAddr("_paged", rows, page_table, page_size)
          the row table {page table offset, position} plus the page table.

    The suffix picks the binding family, which takes `where` in the place
    where the single-sequence bindings take `pos`; only the single-sequence
    attention has scratch of its own to pass."""

    def __init__(self, suffix: str, *where, attn_scratch=()):
        self.rope_kv = "rope_kv" + suffix
        self.rope_kv_qknorm = "rope_kv_qknorm" + suffix
        self.attn = "attn" + suffix
        self.where = where
        self.attn_scratch = attn_scratch
        self.row_table = bool(suffix)  # a row step, not pos..pos+B-1


class HipTransformer:
    # opt-in: capture_decode_graph appends the on-device temperature/top-p
    # sampler to the decode graph (forward_sample); off, nothing changes
    device_sampling = False

    def __init__(self, config: ModelConfig, device=None, comm: Comm | None = None,
                 n_batches: int = 32, force_sync: bool = False,
                 n_slots: int = 1, kv_pages: int = 0, page_size: int = 64,
                 kv_dtype: str | None = None):
        self.cfg = c = config
        if kv_dtype not in (None, "f16", "f32", "q80"):
            raise ValueError(
                f"kv_dtype must be 'f16', 'f32' or 'q80' (got {kv_dtype!r})")
        # KV slots: each layer's cache holds n_slots sequences of seq_len
        # rows; every single-sequence path lives in slot 0 (the first
        # seq_len rows), forward_rows addresses any of them
        if n_slots < 1:
            raise ValueError(f"n_slots must be >= 1 (got {n_slots})")
        self.n_slots = n_slots
        # kv_pages > 0: each layer's cache is a pool of kv_pages pages of
        # page_size rows, and a slot reaches its rows through a page table
        # (set_slot_pages); n_slots then sizes the table, not the memory.
        # A paged model steps rows only.
        self.kv_pages = kv_pages
        self.page_size = page_size
        self.page_map = None
        self.page_table_sends = 0  # copies of table rows to the device
        if kv_pages:
            from .rows import PageMap
            self.page_map = PageMap(n_slots, c.seq_len, kv_pages, page_size)
        self.comm = comm or SingleComm()
        # force_sync: run the full TP sync/gather/concat path at world=1
        # (SingleComm collectives are identity) — lets a 1-GPU box validate
        # every TP kernel and the graph-captured sync step end to end
        self.tp_path = config.world > 1 or force_sync
        self.device = torch.device(device or "cuda")
        self.k = hip_ops()
        # buffers are indexed with NB=_pow2_batch(B) rows and the prefill
        # GEMM's MFMA fragment covers exactly 32 batch rows: a non-pow2 or
        # <32 n_batches would launch grids over short buffers (OOB), and
        # >32 rows would silently never be written by the GEMM. Pin to 32.
        nb = 32
        if n_batches != 32:
            import warnings
            warnings.warn(
                f"HIP backend pins --n-batches to 32 (got {n_batches}): the "
                "prefill GEMM's MFMA fragment is 32 batch rows")
        self.n_batches = nb
        self.layers: list[dict] = []
        self.embedding = None
        self.final_norm = None
        self.wcls = None
        # every captured graph, valid at the attn_splits in force
        # (no reference back to the model: a cycle would leave a dropped
        # model, graphs and all, to a garbage collection mid-capture)
        self.graphs = StepGraphs(partial(capture_hip_graph, self.device),
                                 on_gpu=self.device.type == "cuda")
        self._graph_pos = None      # where the decode graph left the device pos
        self._graph_wanted = False  # capture_decode_graph was asked for
        self.row_graphs = True      # capture all-decode forward_rows steps
        # token log-probabilities (set_logprobs): off by default; part of
        # a graph's key, so switching recaptures nothing
        self.logprobs = False
        self._lp_scratch = None
        self._lp_host = None        # what the last step's one copy brought
        self._lp_rows_host = None
        self._dev_sampler = None
        self.greedy_feedback = False
        self.skip_logits = False  # prefill chunks before the last skip wcls
        self._rows_io = None      # row-step staging, built on first use
        # per-model constants
        self.kv_mul = c.n_heads0 // max(1, c.kv_dim0 // c.head_dim)
        self.rope_style = 1 if c.rope_type == ROPE_FALCON else 0
        self.fused_rope = self.rope_style == 0 and not c.is_qwen3
        self.row_bytes = c.dim + 2 * (c.dim // QB)  # one Q80 wire row
        self._read_options()
        # KV cache format: None = f16, or f32 under DLLAMA_KV_F32=1; an
        # explicit value wins over the environment. "q80": int8 codes + f16
        # block scales, 0.53x the bytes of f16 (docs/DESIGN.md §8).
        self.kv_dtype = kv_dtype or ("f32" if self.kv_f32 else "f16")
        self.kv_f32 = self.kv_dtype == "f32"
        self.kv_q80 = self.kv_dtype == "q80"
        if self.kv_q80:
            # the GEMV rope epilogue holds two rows per wave and cannot see
            # a Q80 block: the QKV GEMV + rope_kv pair runs instead (one more
            # launch per layer for a single llama sequence)
            self.fused_rope = False
        self._alloc_buffers()

    def _read_options(self):
        """Every DLLAMA_* option of the model, read once per construction."""
        env = os.environ

        def flag(name: str, default: str) -> bool:
            return env.get(name, default) == "1"

        self.attn_splits = int(env.get("DLLAMA_ATTN_SPLITS", "8"))
        # fused quantize-into-wire sync: validated bit-identical on hardware
        # (test_sync_quant_pack_matches_two_kernel_path); default on
        self.fused_sync = flag("DLLAMA_FUSED_SYNC", "1")
        # adaptive K-split schedule: S=1 (the wide single-launch attention,
        # no combine launch) below wide_thresh, S=8 to the threshold, S=16
        # beyond (tools/attn_kv16_probe: S=16 wins from ~pos 512). The decode
        # graph is recaptured when pos crosses a boundary.
        # DLLAMA_ADAPTIVE_SPLITS=0 (or an explicit DLLAMA_ATTN_SPLITS) pins S.
        self.adaptive_thresh = int(env.get("DLLAMA_ADAPTIVE_SPLITS", "512"))
        if ("DLLAMA_ATTN_SPLITS" in env
                and "DLLAMA_ADAPTIVE_SPLITS" not in env):
            self.adaptive_thresh = 0
        # positions below this take the wide kernel: the measured crossover
        # against the best split + combine pair, rounded down to a multiple
        # of the kernel's 256-timestep round (profiles/r07_wide_attention.md).
        # DLLAMA_ATTN_WIDE=<pos> moves it, 0 turns the tier off.
        self.wide_thresh = int(env.get("DLLAMA_ATTN_WIDE", "256"))
        # row steps (forward_rows) take the tier on request: set_wide_rows,
        # which BatchEngine calls, or DLLAMA_ATTN_WIDE_ROWS=1
        self.wide_rows = flag("DLLAMA_ATTN_WIDE_ROWS", "0")
        # the S in force above the wide tier, put back when a step leaves it
        self._splits_above = self.attn_splits if self.attn_splits != 1 else 8
        # measured-slower fusions kept for shape experiments (profiles r02):
        # the 16-wave fused FFN streams worse than the 4-wave GEMV + swiglu
        # pair, and per-wave gate recompute adds ~8 us to each MoE consumer
        self.fused_ffn = flag("DLLAMA_FUSED_FFN", "0")
        self.fused_moe = flag("DLLAMA_FUSED_MOE", "0")
        # deferred-quant dense decode (EPI_RESID_Q + PRO2); =0 reverts to
        # explicit norm_quant launches
        self.use_deferred = flag("DLLAMA_DEFERRED", "1")
        # bf16 prefill: dense prompt chunks run hipBLASLt GEMMs (torch.mm)
        # over a bf16 copy of the weights. Measured SLOWER than the
        # hand-written int8-MFMA GEMM at the 32-token chunk shape (5355 vs
        # 5651 tok/s prefill) and costs a 2x-weight shadow — off by default,
        # kept as the library baseline for GEMM tuning A/Bs.
        self.prefill_bf16 = flag("DLLAMA_PREFILL_BF16", "0")
        # K-split the deferred down-projections (wo/w2 underfill at 1 wg per
        # 32 rows when dim <= 4096); merged by add_ssq_q. A/B experiment.
        self.ksplit_resid = int(env.get("DLLAMA_KSPLIT_RESID", "0"))
        # f16 KV cache by default: halves the attention HBM stream (measured
        # 1.45x at 1k ctx, 1.7x at 4k — tools/attn_kv16_probe; maxerr ~2e-5
        # vs f32). DLLAMA_KV_F32=1 reverts to the reference's f32 layout.
        self.kv_f32 = flag("DLLAMA_KV_F32", "0")

    # ------------------------------------------------------------ weights

    @classmethod
    def from_file(cls, m: ModelFile, config: ModelConfig, device=None,
                  comm: Comm | None = None, n_batches: int = 32,
                  force_sync: bool = False,
                  n_slots: int = 1, kv_pages: int = 0,
                  page_size: int = 64,
                  kv_dtype: str | None = None) -> "HipTransformer":
        from ..quants import Q40
        if m.header.weight_type != Q40:
            raise ValueError(
                "the MI355X HIP backend runs Q40 weights (the reference's "
                "shipped format); f32/q80 .m files run on the CPU backend "
                "(--gpu-index -1) or can be re-quantized with convert_hf.py")
        self = cls(config, device, comm, n_batches, force_sync, n_slots,
                   kv_pages, page_size, kv_dtype)
        c, dev = config, self.device
        r, w = c.rank, c.world

        def lin(name, layer, d, n, expert=-1):
            e = m.entry(name, layer, expert)
            raw = m.slice_bytes(e, r, w)
            return Linear.from_blocks(raw, d, n, dev)

        def f32(name, layer=-1):
            return torch.from_numpy(np.array(m.f32(name, layer))).to(dev)

        def w13(l, expert=-1):
            return Linear.cat(lin("block_matmul_w1", l, c.ff_dim0, c.dim, expert),
                              lin("block_matmul_w3", l, c.ff_dim0, c.dim, expert))

        self.embedding = f32("embedding")
        self.final_norm = f32("final_norm")
        self.wcls = lin("final_matmul_logits", -1, c.vocab0, c.dim)
        for l in range(c.n_layers):
            # fuse Q|K|V (and W1|W3) into single GEMV weights: one launch,
            # one pass over x, full-chip grids even for the small K/V shards
            lw = {
                "qkv": Linear.cat(lin("block_matmul_q", l, c.q_dim0, c.dim),
                                  lin("block_matmul_k", l, c.kv_dim0, c.dim),
                                  lin("block_matmul_v", l, c.kv_dim0, c.dim)),
                "wo": lin("block_matmul_wo", l, c.dim, c.q_dim0),
                "norm0": f32("block_norm_0", l),
                "norm1": f32("block_norm_1", l),
            }
            if c.is_moe:
                experts = range(c.n_experts)
                lw["gate"] = f32("block_moe_gate", l)
                lw["w13"] = Linear.stack([w13(l, e) for e in experts])
                lw["w2"] = Linear.stack(
                    [lin("block_matmul_w2", l, c.dim, c.ff_dim0, e)
                     for e in experts])
            else:
                lw["w13"] = w13(l)
                lw["w2"] = lin("block_matmul_w2", l, c.dim, c.ff_dim0)
            if c.is_qwen3:
                lw["q_norm"] = f32("block_norm_q", l)
                lw["k_norm"] = f32("block_norm_k", l)
            self.layers.append(lw)
        self._finish_init()
        return self

    @classmethod
    def synthetic(cls, config: ModelConfig, device=None, comm: Comm | None = None,
                  n_batches: int = 32, seed: int = 1234,
                  force_sync: bool = False,
                  n_slots: int = 1, kv_pages: int = 0,
                  page_size: int = 64,
                  kv_dtype: str | None = None) -> "HipTransformer":
        """Random-init weights built directly on device (benches: no network
        for checkpoints, and an 8B .m file round-trip is pointless there)."""
        self = cls(config, device, comm, n_batches, force_sync, n_slots,
                   kv_pages, page_size, kv_dtype)
        c, dev = config, self.device
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed + c.rank)
        experts = c.n_experts if c.is_moe else None
        self.embedding = torch.randn(c.vocab_size, c.dim, device=dev,
                                     generator=gen) * 0.02
        self.final_norm = torch.ones(c.dim, device=dev)
        self.wcls = Linear.synthetic(c.vocab0, c.dim, dev, gen)
        for l in range(c.n_layers):
            # the draw order below fixes the weights: keep it
            lw = {
                "qkv": Linear.synthetic(c.q_dim0 + 2 * c.kv_dim0, c.dim, dev, gen),
                "wo": Linear.synthetic(c.dim, c.q_dim0, dev, gen),
                "norm0": torch.ones(c.dim, device=dev),
                "norm1": torch.ones(c.dim, device=dev),
            }
            if c.is_moe:
                lw["gate"] = torch.randn(c.n_experts, c.dim, device=dev,
                                         generator=gen) * 0.02
            lw["w13"] = Linear.synthetic(2 * c.ff_dim0, c.dim, dev, gen,
                                         experts=experts)
            lw["w2"] = Linear.synthetic(c.dim, c.ff_dim0, dev, gen,
                                        experts=experts)
            if c.is_qwen3:
                lw["q_norm"] = torch.ones(c.head_dim, device=dev)
                lw["k_norm"] = torch.ones(c.head_dim, device=dev)
            self.layers.append(lw)
        self._finish_init()
        return self

    def _alloc_buffers(self):
        c, dev, NB = self.cfg, self.device, self.n_batches
        self.pos = torch.zeros(1, dtype=torch.int32, device=dev)
        # one allocation for what the host sends per decode step: the token
        # ids, then the sampler's f64 {coin, temperature, topp, unused}, so
        # forward_sample stages both with a single small copy
        self._step_in = torch.zeros(NB + 4, dtype=torch.int64, device=dev)
        self.tokens = self._step_in[:NB]
        self.sample_params = self._step_in[NB:].view(torch.float64)
        # what one step hands back, in one allocation so one copy returns
        # it: {token, status}, then (set_logprobs) the row's f32 {lse,
        # logprob, top-20 logprobs} and its i32 top-20 ids
        self._sample_io = torch.zeros(LP_WORDS, dtype=torch.int64, device=dev)
        self.sample_out = self._sample_io[:2]  # token, status
        self.x = torch.zeros(NB, c.dim, device=dev)
        self.t_norm = torch.zeros(NB, c.dim, device=dev)
        self.xq = QuantBuf(NB, c.dim, dev)
        self.qkv_ld = c.q_dim0 + 2 * c.kv_dim0
        self.qkv_out = torch.zeros(NB, self.qkv_ld, device=dev)
        self.zbuf = torch.zeros(NB, c.q_dim0, device=dev)
        self.zq = QuantBuf(NB, c.q_dim0, dev)
        self.partial = torch.zeros(NB, c.dim, device=dev)
        self.ff_out = torch.zeros(NB, 2 * c.ff_dim0, device=dev)
        self.dq = QuantBuf(NB, c.ff_dim0, dev)
        self.logits0 = torch.zeros(NB, c.vocab0, device=dev)
        rpw = 2 if c.vocab0 >= 2048 else 1
        self.amax_blocks = -(-c.vocab0 // (4 * rpw))  # mirrors gemv RPW choice
        self.gemm_part = torch.zeros(32 * 32 * 8192, device=dev)  # K-split partials
        # sum-of-squares accumulators: [slot, batch, 16 spread x 32 pad]
        # (16 slots each on their own cacheline; atomics to one line serialize)
        self.ssq = torch.zeros(2 * c.n_layers + 1, NB, 16 * 32, device=dev)
        self.amax_scratch = torch.zeros(self.amax_blocks, dtype=torch.int64, device=dev)
        self._alloc_attn_scratch()
        self.attn_counter = torch.zeros(NB * c.n_heads0, dtype=torch.int32, device=dev)
        self.seq_addr = KVAddr("", self.pos, attn_scratch=(self.attn_counter,))
        if self.tp_path:
            # per-batch-size contiguous gather buffers: collectives need a
            # flat contiguous output (world, nb*...) — a [:, :nb] slice is not
            nbs = [n for n in (1, 2, 4, 8, 16, 32) if n <= NB]
            self.logits_gather = {n: torch.zeros(c.world, n, c.vocab0, device=dev)
                                  for n in nbs}
            self.logits_full = torch.zeros(NB, c.world * c.vocab0, device=dev)
            self.argmax_scratch_full = torch.zeros(
                -(-c.world * c.vocab0 // 4096), dtype=torch.int64, device=dev)
            if c.sync_type == Q80:
                self.sync_out = torch.zeros(NB * self.row_bytes,
                                            dtype=torch.uint8, device=dev)
                self.sync_in = {n: torch.zeros(c.world, n * self.row_bytes,
                                               dtype=torch.uint8, device=dev)
                                for n in nbs}
        if c.is_moe:
            S = NB * c.n_active_experts
            self.moe_idx = torch.zeros(S, dtype=torch.int32, device=dev)
            self.moe_wts = torch.zeros(NB, c.n_active_experts, device=dev)
            self.moe_router = torch.zeros(NB, c.n_experts, device=dev)
            self.moe_out13 = torch.zeros(S, 2 * c.ff_dim0, device=dev)
            self.moe_dq = QuantBuf(S, c.ff_dim0, dev)
            self.moe_y = torch.zeros(S, c.dim, device=dev)

    def _alloc_attn_scratch(self):
        """Flash-decode split scratch sized for the current S (the adaptive
        schedule reallocates on recapture: 8 short ctx, 16 past 512, 32
        past 2k)."""
        c, dev = self.cfg, self.device
        n = self.n_batches * c.n_heads0 * self.attn_splits
        self.attn_ml = torch.zeros(n * 2, device=dev)
        self.attn_o = torch.zeros(n * c.head_dim, device=dev)

    def _dequant_bf16(self, lin: Linear) -> torch.Tensor:
        """Q40 planes -> bf16 weight matrix on device (prefill GEMM shadow;
        same dequantized values the int8 GEMV streams, rounded to bf16)."""
        qs = lin.qs
        d, nb2 = qs.shape[-2], qs.shape[-1]
        n = nb2 * 2
        lo = (qs & 15).to(torch.float32) - 8.0
        hi = (qs >> 4).to(torch.float32) - 8.0
        lo = lo.view(*qs.shape[:-1], n // 32, 16)
        hi = hi.view(*qs.shape[:-1], n // 32, 16)
        w = torch.cat([lo, hi], dim=-1)  # elems j | j+16 per block
        sc = lin.scales.view(*qs.shape[:-1], n // 32, 1).float()
        return (w * sc).view(*qs.shape[:-2], d, n).to(torch.bfloat16)

    def _build_bf16_shadow(self):
        """bf16 copies of the dense matmul weights for hipBLASLt prefill
        (skipped for MoE/TP where the Q40 GEMM path stays)."""
        c = self.cfg
        if not self.prefill_bf16 or c.is_moe or self.tp_path:
            self.prefill_bf16 = False
            return
        self.wcls_bf16 = self._dequant_bf16(self.wcls)
        for lw in self.layers:
            lw["qkv_bf16"] = self._dequant_bf16(lw["qkv"])
            lw["wo_bf16"] = self._dequant_bf16(lw["wo"])
            lw["w13_bf16"] = self._dequant_bf16(lw["w13"])
            lw["w2_bf16"] = self._dequant_bf16(lw["w2"])

    def _finish_init(self):
        c, dev = self.cfg, self.device
        self._build_bf16_shadow()
        cache = R.rope_cache(c.seq_len, c.head_dim, c.rope_theta, c.rope_scaling)
        self.rope_cache = cache.reshape(c.seq_len, c.head_dim).contiguous().to(dev)
        kv_dt = (torch.int8 if self.kv_q80
                 else torch.float32 if self.kv_f32 else torch.float16)
        kv_rows = self.n_slots * c.seq_len  # slot s = rows s*seq_len ...
        if self.page_map is not None:
            kv_rows = self.kv_pages * self.page_size
            # unmapped entries hold 0: the table never points outside the pool
            self.page_table = torch.zeros(
                self.n_slots, self.page_map.pages_per_seq, dtype=torch.int32,
                device=dev)
        self.k_cache = [torch.zeros(kv_rows, c.kv_dim0, dtype=kv_dt, device=dev)
                        for _ in range(c.n_layers)]
        self.v_cache = [torch.zeros(kv_rows, c.kv_dim0, dtype=kv_dt, device=dev)
                        for _ in range(c.n_layers)]
        if self.kv_q80:
            # the scale planes, indexed by the same cache row as the codes;
            # zero codes and zero scales dequantise to 0 like an empty cache
            def scales():
                return [torch.zeros(kv_rows, c.kv_dim0 // QB,
                                    dtype=torch.float16, device=dev)
                        for _ in range(c.n_layers)]
            self.k_scales, self.v_scales = scales(), scales()

    def _kv_scales(self, l: int) -> dict:
        """The keywords that hand layer l's scale planes to a positional
        binding; none unless the cache is Q80."""
        if not self.kv_q80:
            return {}
        return {"k_scales": self.k_scales[l], "v_scales": self.v_scales[l]}

    def kv_cache_bytes(self) -> int:
        """Bytes of all K/V planes of all layers (scale planes included)."""
        planes = self.k_cache + self.v_cache
        if self.kv_q80:
            planes = planes + self.k_scales + self.v_scales
        return sum(t.numel() * t.element_size() for t in planes)

    # ------------------------------------------------------------ stages

    def _norm_quant(self, wn, slot: int, NB: int, *out_f32, **kw):
        """x[:NB] * wn * inv_rms(ssq[slot]) -> Q80 triple in xq."""
        self.k.norm_quant(self.x[:NB], wn, self.ssq[slot], *self.xq.triple(NB),
                          NB, self.cfg.norm_eps, *out_f32, **kw)

    def _mm(self, lin: Linear, qb: QuantBuf, out, NB: int, amax=None):
        """Batched matmul dispatch: decode batches use the dot4 GEMV,
        prefill batches (>=8) the int8-MFMA GEMM."""
        if NB >= 8:
            self.k.q40_gemm(lin.qs, lin.scales, qb.q, qb.s, out, NB,
                            self.gemm_part)
        else:
            self.k.q40_gemv(lin.qs, lin.scales, *qb.triple(), out, NB, amax)

    def _norm_mm(self, lin: Linear, wn, slot: int, out, NB: int, amax=None):
        """Normed + quantized x -> matmul. (A norm+quant GEMV prologue was
        measured VALU-bound, 2x slower on the big GEMVs: x is re-quantized
        per workgroup.)"""
        self._norm_quant(wn, slot, NB)
        self._mm(lin, self.xq, out, NB, amax)

    def _gemv_rope(self, l: int, lw: dict, NB: int, **deferred):
        """QKV GEMV with llama rope + KV write in its epilogue."""
        c = self.cfg
        assert not self.kv_q80, "the rope epilogue has no Q80 cache form"
        self.k.q40_gemv_rope(lw["qkv"].qs, lw["qkv"].scales, *self.xq.triple(),
                             self.qkv_out, NB, self.rope_cache, self.pos,
                             self.k_cache[l], self.v_cache[l], c.q_dim0,
                             c.kv_dim0, c.head_dim, **deferred)

    def _qknorm_rope_kv(self, l: int, lw: dict, B: int, addr: KVAddr):
        """Per-head q/k rmsnorm (qwen3), rope and KV write on qkv_out, for
        the schedules whose QKV matmul has no rope epilogue."""
        c, k = self.cfg, self.k
        if c.is_qwen3 and self.rope_style == 1:
            # one launch (replaces 2x rmsnorm_rows_s + rope_kv = ~9 us/layer
            # of launch overhead in the captured graph)
            getattr(k, addr.rope_kv_qknorm)(
                self.qkv_out, self.qkv_ld, c.q_dim0, c.kv_dim0,
                self.rope_cache, *addr.where, self.k_cache[l],
                self.v_cache[l], c.head_dim, lw["q_norm"], lw["k_norm"],
                c.norm_eps, B, **self._kv_scales(l))
            return
        if c.is_qwen3:
            for col0, width, wn in ((0, c.q_dim0, lw["q_norm"]),
                                    (c.q_dim0, c.kv_dim0, lw["k_norm"])):
                k.rmsnorm_rows_s(self.qkv_out, self.qkv_ld, col0,
                                 width // c.head_dim, B, wn, c.head_dim,
                                 c.norm_eps)
        getattr(k, addr.rope_kv)(
            self.qkv_out, self.qkv_ld, c.q_dim0, c.kv_dim0, self.rope_cache,
            *addr.where, self.k_cache[l], self.v_cache[l], c.head_dim,
            self.rope_style, B, **self._kv_scales(l))

    def _attn(self, l: int, B: int, addr: KVAddr, emit_q80: bool = True):
        """Attention of every row over its sequence's rows of layer l's
        cache into zbuf[:B]; emit_q80 also writes the Q80 triple zq that the
        wo matmul consumes."""
        c = self.cfg
        getattr(self.k, addr.attn)(
            self.qkv_out, self.qkv_ld, self.k_cache[l], self.v_cache[l],
            self.zbuf[:B], *addr.where, B, c.n_heads0, self.kv_mul,
            c.head_dim, self.attn_splits, self.attn_ml, self.attn_o,
            *addr.attn_scratch, *(self.zq.triple() if emit_q80 else ()),
            **self._kv_scales(l))

    def _swiglu_q80(self, out13, rows: int, qb: QuantBuf, *act):
        """act(w1 x) * (w3 x) over the fused W1|W3 output -> Q80 triple."""
        f = self.cfg.ff_dim0
        self.k.swiglu_q80(out13, out13[:, f:], 2 * f, f, rows,
                          *qb.triple(rows), *act)

    def _wire_exchange(self, n: int, ssq_slot, wnorm=None):
        """Q80 wire sync, given this rank's n packed rows in sync_out:
        all-gather, then merge-add every rank's slice into x[:n] with the
        row sum-of-squares into ssq_slot. With wnorm the merge also emits
        the next matmul's deferred quant into xq."""
        c = self.cfg
        inb = self.sync_in[n]
        self.comm.all_gather(inb, self.sync_out[: n * self.row_bytes])
        wire = inb.view(c.world, n, self.row_bytes)
        if wnorm is None:
            self.k.merge_add(self.x[:n], wire, ssq_slot)
        else:
            self.k.merge_add_q(self.x[:n], wire, ssq_slot, wnorm,
                               *self.xq.triple())

    def _sync_partial(self, NB: int, slot: int):
        """TP>1: all-reduce self.partial[:NB] into x (+= sum of partials),
        accumulating the residual row's sum-of-squares into ssq[slot]."""
        k = self.k
        if self.cfg.sync_type != Q80:
            self.comm.allreduce_(self.partial[:NB])
            k.add_ssq(self.x[:NB], self.partial[:NB], self.ssq[slot], NB)
            return
        out = self.sync_out[: NB * self.row_bytes]
        if self.fused_sync:
            # quantize straight into the wire buffer, one pass
            # (default; DLLAMA_FUSED_SYNC=0 splits it)
            k.sync_quant_pack(self.partial[:NB], out)
        else:
            q, s, bs = self.xq.triple(NB)  # reuse dim-sized quant buffer
            k.q80_quantize(self.partial[:NB], q, s, bs)
            k.sync_pack(q, s, out)
        self._wire_exchange(NB, self.ssq[slot])

    def _proj_merge(self, lin: Linear, qb: QuantBuf, slot: int, NB: int):
        """Down-projection + residual fold: TP=1 decode fuses the add + ssq
        into the GEMV epilogue (+1us with cacheline-strided ssq slots — the
        earlier +6.5us was atomics serializing on one cacheline)."""
        k = self.k
        if not self.tp_path and NB < 8:
            k.q40_gemv_resid(lin.qs, lin.scales, *qb.triple(),
                             self.x, self.ssq[slot], NB)
            return
        self._mm(lin, qb, self.partial, NB)
        if not self.tp_path:
            k.add_ssq(self.x[:NB], self.partial[:NB], self.ssq[slot], NB)
        else:
            self._sync_partial(NB, slot)

    def _proj_merge_deferred(self, lin: Linear, qb: QuantBuf, slot: int, wnorm):
        """B=1 down-projection + residual fold into x and ssq[slot], which
        also emits x*wnorm as the next matmul's deferred Q80 input in xq.
        TP: the GEMV epilogue packs the Q80 wire instead and the merge-add
        after the all-gather folds the residual and emits the quant
        (reference SYNC_NODE_SLICES + OP_MERGE_ADD, one fewer launch on
        each side of the collective)."""
        k, ssq = self.k, self.ssq[slot]
        if self.tp_path:
            k.q40_gemv_pack(lin.qs, lin.scales, *qb.triple(),
                            self.sync_out[: self.row_bytes])
            self._wire_exchange(1, ssq, wnorm)
        elif self.ksplit_resid:
            k.q40_gemv_ksplit(lin.qs, lin.scales, *qb.triple(),
                              self.gemm_part, self.ksplit_resid)
            k.add_ssq_q(self.x[:1], self.gemm_part, ssq, wnorm,
                        *self.xq.triple(1), self.ksplit_resid)
        else:
            k.q40_gemv_resid_q(lin.qs, lin.scales, *qb.triple(), self.x, ssq,
                               wnorm, *self.xq.triple())

    def _logits(self, B: int, NB: int, slot: int, deferred: bool = False,
                feedback: bool = True):
        """wcls matmul over the final norm, TP gather of the vocab shards,
        and (greedy_feedback, B=1) the on-device argmax into tokens[0];
        feedback=False leaves tokens alone whatever greedy_feedback says."""
        c, k = self.cfg, self.k
        greedy = self.greedy_feedback and B == 1 and feedback
        use_amax = greedy and not self.tp_path
        amax = self.amax_scratch if use_amax else None
        if deferred:
            k.q40_gemv(self.wcls.qs, self.wcls.scales, *self.xq.triple(),
                       self.logits0, 1, amax, ssq_in=self.ssq[slot],
                       eps=c.norm_eps)
        else:
            self._norm_mm(self.wcls, self.final_norm, slot, self.logits0, NB,
                          amax)
        if self.tp_path:
            self.comm.all_gather(self.logits_gather[NB], self.logits0[:NB])
        if not greedy:
            return
        # on-device greedy sampling feeding the next decode step (used by
        # the fully graph-captured bench loop; real serving samples after
        # forward_buffers: the sampler kernels with device_sampling, else
        # on host)
        if use_amax:
            k.token_from_argmax(self.tokens, self.amax_scratch, self.amax_blocks)
        else:
            # TP: gathered slices are contiguous in global vocab order
            # (row-split wcls), so the flat gather buffer IS the full
            # logits row; two-kernel argmax, no ATen in the graph
            k.argmax_token(self.tokens, self.logits_gather[1].view(-1),
                           self.argmax_scratch_full)

    # ------------------------------------------------------------ forward

    def forward_buffers(self, B: int):
        """Run one step over tokens[:B] at positions pos..pos+B-1, writing
        logits into logits0 (and the gather buffer under TP). Everything
        stays on device — this function is graph-capturable."""
        c = self.cfg
        tp_def_ok = (not self.tp_path
                     or (c.sync_type == Q80 and c.dim % 256 == 0))
        if (B == 1 and c.dim % 32 == 0 and tp_def_ok
                and (not c.is_moe
                     or (c.dim % 256 == 0 and c.n_active_experts <= 16))
                and self.use_deferred):
            return self._forward_dense_deferred()
        if B >= 8 and self.prefill_bf16:
            return self._forward_prefill_bf16(B)
        self._forward_explicit(B, self.seq_addr)

    def _forward_explicit(self, B: int, addr: KVAddr):
        """The explicit-norm schedule (norm_quant in front of every matmul)
        over B rows under any addressing. All K/V rows of a step are written
        before its attention launches, so rows of one sequence (a prompt
        chunk) see each other.

        A row step (addr.row_table) differs from the single-sequence step
        in five conditions below. Four follow from what a row step is:
          - its tokens arrive in row_tokens, staged with the table in one
            copy;
          - the QKV GEMV with the rope epilogue reads `pos` and has no
            row-table form, so the separate rope/KV launch always runs;
          - its rows belong to different sequences that each sample from
            their own logits row, so the logits are always computed, and
            greedy feedback (an argmax into tokens[0], which a row step
            does not read) never runs;
          - under TP the vocab shards are concatenated inside the step,
            where a captured row graph's per-row samplers read them; the
            single-sequence caller (`forward`) does it after the step.
        One is history only: a one-row step could take the fused FFN GEMV,
        but DLLAMA_FUSED_FFN (measured slower) was never wired to row
        steps, and the pinned launch traces keep it that way."""
        c, k = self.cfg, self.k
        NB = _pow2_batch(B)
        rows = addr.row_table
        self.ssq.zero_()
        k.embed_gather(self.embedding, self.row_tokens if rows else self.tokens,
                       self.x, NB, self.ssq[0])
        slot = 0
        for l, lw in enumerate(self.layers):
            # attention block
            if self.fused_rope and NB < 8 and not rows:
                self._norm_quant(lw["norm0"], slot, NB)
                self._gemv_rope(l, lw, NB)
            else:
                self._norm_mm(lw["qkv"], lw["norm0"], slot, self.qkv_out, NB)
                self._qknorm_rope_kv(l, lw, B, addr)
            self._attn(l, B, addr)
            self._proj_merge(lw["wo"], self.zq, slot + 1, NB)
            slot += 1

            # ffn block
            if c.is_moe:
                # norm once: Q80 triple for the expert GEMVs + f32 for router
                self._norm_quant(lw["norm1"], slot, NB, self.t_norm[:NB])
                self._moe_ffn(B, NB, lw, slot + 1)
            else:
                gelu = c.hidden_act == HIDDEN_ACT_GELU
                if (NB == 1 and c.ff_dim0 % 32 == 0 and self.fused_ffn
                        and not rows):
                    # fused W1|W3 GEMV + SwiGLU + Q80 emit (one launch
                    # replacing gemv + swiglu_q80)
                    self._norm_quant(lw["norm1"], slot, NB)
                    k.q40_gemv_swiglu(lw["w13"].qs, lw["w13"].scales,
                                      *self.xq.triple(), *self.dq.triple(),
                                      gelu)
                else:
                    self._norm_mm(lw["w13"], lw["norm1"], slot, self.ff_out, NB)
                    self._swiglu_q80(self.ff_out, NB, self.dq, gelu)
                self._proj_merge(lw["w2"], self.dq, slot + 1, NB)
            slot += 1

        if self.skip_logits and B > 1 and not rows:
            return
        self._logits(B, NB, slot, feedback=not rows)
        if rows and self.tp_path:
            k.logits_concat(self.logits_full, self.logits_gather[NB], B)

    def _forward_prefill_bf16(self, B: int):
        """Dense prompt chunks as hipBLASLt bf16 GEMMs over the weight
        shadow: prefill is batch>=8 plain GEMM work, which belongs on the
        matrix cores — the hand-written Q40 int8 GEMM is VALU-bound at
        ~1.3 TB/s weight stream while the bf16 library GEMM is MFMA-bound
        (the reference's llamafile sgemm plays this exact role for batch>1,
        src/nn/llamafile/sgemm.cpp:819-986). rope/KV/attention/norm stay in
        the HIP kernels; elementwise glue is torch (prefill runs once per
        32-token chunk, not per token)."""
        import torch.nn.functional as F
        c, k = self.cfg, self.k
        NB = _pow2_batch(B)
        x = self.x

        def norm_mm(wn, slot, w_bf16):
            k.norm_f32(x[:NB], wn, self.ssq[slot], self.t_norm[:NB], NB,
                       c.norm_eps)
            return torch.mm(self.t_norm[:NB].bfloat16(), w_bf16.t())

        self.ssq.zero_()
        k.embed_gather(self.embedding, self.tokens, x, NB, self.ssq[0])
        slot = 0
        for l, lw in enumerate(self.layers):
            self.qkv_out[:NB].copy_(norm_mm(lw["norm0"], slot, lw["qkv_bf16"]))
            self._qknorm_rope_kv(l, lw, B, self.seq_addr)
            self._attn(l, B, self.seq_addr, emit_q80=False)
            partial = torch.mm(self.zbuf[:NB].bfloat16(),
                               lw["wo_bf16"].t()).float()
            k.add_ssq(x[:NB], partial, self.ssq[slot + 1], NB)
            slot += 1
            ff = norm_mm(lw["norm1"], slot, lw["w13_bf16"]).float()
            a, g = ff[:, :c.ff_dim0], ff[:, c.ff_dim0:]
            if c.hidden_act == HIDDEN_ACT_GELU:
                d = F.gelu(a, approximate="tanh") * g
            else:
                d = F.silu(a) * g
            partial = torch.mm(d.bfloat16(), lw["w2_bf16"].t()).float()
            k.add_ssq(x[:NB], partial, self.ssq[slot + 1], NB)
            slot += 1
        if self.skip_logits and B > 1:
            return
        self.logits0[:NB].copy_(norm_mm(self.final_norm, slot, self.wcls_bf16))

    def _forward_dense_deferred(self):
        """B=1 decode with DEFERRED activation quantization: the
        down-projection GEMVs emit the next matmul's Q80 input in their own
        epilogue (x*w_norm quantized per wg-local block, scale excluding
        inv_rms), and every consumer GEMV applies inv = rsqrt(ssq/n + eps)
        as one multiply per output row. This removes both norm_quant
        launches per layer — the Q80 codes are scale-invariant, so numerics
        match the explicit-norm path to fp rounding (reference runs
        merge_add/inv_rms/rms_norm/cast as 4 ops per half-layer,
        llm.cpp:263-270)."""
        c, k = self.cfg, self.k
        eps = c.norm_eps
        self.ssq.zero_()
        k.embed_gather(self.embedding, self.tokens, self.x, 1, self.ssq[0])
        # layer 0's norm0 quant comes from a deferred norm_quant (later
        # layers get it from the previous w2's EPI_RESID_Q epilogue)
        self._norm_quant(self.layers[0]["norm0"], 0, 1, deferred=True)
        slot = 0
        last = len(self.layers) - 1
        for l, lw in enumerate(self.layers):
            sin = self.ssq[slot]
            if self.fused_rope:
                self._gemv_rope(l, lw, 1, ssq_in=sin, eps=eps)
            else:
                k.q40_gemv(lw["qkv"].qs, lw["qkv"].scales, *self.xq.triple(),
                           self.qkv_out, 1, ssq_in=sin, eps=eps)
                self._qknorm_rope_kv(l, lw, 1, self.seq_addr)
            self._attn(l, 1, self.seq_addr)
            # wo: residual fold + deferred Q80 emit of x*norm1 for the FFN
            self._proj_merge_deferred(lw["wo"], self.zq, slot + 1, lw["norm1"])
            slot += 1
            # the FFN's fold emits the NEXT layer's norm0 quant (final_norm
            # for logits after the last layer)
            wn = self.final_norm if l == last else self.layers[l + 1]["norm0"]
            if c.is_moe:
                self._moe_ffn_deferred(lw, slot, wn)
            else:
                k.q40_gemv(lw["w13"].qs, lw["w13"].scales, *self.xq.triple(),
                           self.ff_out, 1, ssq_in=self.ssq[slot], eps=eps)
                self._swiglu_q80(self.ff_out, 1, self.dq,
                                 c.hidden_act == HIDDEN_ACT_GELU)
                self._proj_merge_deferred(lw["w2"], self.dq, slot + 1, wn)
            slot += 1
        self._logits(1, 1, slot, deferred=True)

    def _moe_ffn_deferred(self, lw: dict, slot: int, wn):
        """MoE deferred FFN: router reads x*norm1*inv directly (no t_norm
        buffer), grouped w13 consumes the deferred xq, and the scale-merge
        epilogue emits the NEXT layer's deferred quant — both per-layer
        norm_quant launches gone here too."""
        c, k = self.cfg, self.k
        ka = c.n_active_experts
        k.router_gemv_norm(lw["gate"], self.x, lw["norm1"], self.ssq[slot],
                           c.norm_eps, self.moe_router, 1)
        k.moe_gate(self.moe_router[:1], self.moe_idx, self.moe_wts, 1, ka)
        k.q40_gemv_grouped(lw["w13"].qs, lw["w13"].scales, *self.xq.triple(),
                           self.moe_idx[:ka], self.moe_out13, ka,
                           ssq_in=self.ssq[slot], eps=c.norm_eps)
        self._swiglu_q80(self.moe_out13, ka, self.moe_dq)
        k.q40_gemv_grouped(lw["w2"].qs, lw["w2"].scales, *self.moe_dq.triple(),
                           self.moe_idx[:ka], self.moe_y, 1)
        if self.tp_path:
            # expert-weighted sum packed straight into the Q80 wire;
            # merge-add after the gather folds residual + emits the next
            # deferred quant
            k.scale_merge_pack(self.moe_y, self.moe_wts,
                               self.sync_out[: self.row_bytes], 1, ka, c.dim)
            self._wire_exchange(1, self.ssq[slot + 1], wn)
        else:
            k.scale_merge_add_q(self.x[:1], self.moe_y, self.moe_wts,
                                self.ssq[slot + 1], wn, *self.xq.triple(),
                                1, ka)

    def _moe_ffn(self, B: int, NB: int, lw: dict, slot: int):
        """Router + grouped expert GEMVs (reference llm.cpp:450-487);
        t_norm holds the f32 normed activations (router input), xq the same
        values Q80-quantized (expert GEMV input = reference repeat_z)."""
        c, k = self.cfg, self.k
        ka = c.n_active_experts
        S = NB * ka
        k.router_gemv(lw["gate"], self.t_norm, self.moe_router, NB)
        if c.ff_dim0 % 32 == 0 and ka <= 16 and self.fused_moe:
            # gate-fused decode path: every consumer recomputes the
            # deterministic top-k from the router logits in-kernel, so the
            # FFN is 3 launches (w13+swiglu, w2, scale-merge) instead of 6
            # and the merge takes the router logits for the expert weights
            wts, gate = self.moe_router[:NB], {"gate": True}
            k.q40_gemv_grouped_swiglu(lw["w13"].qs, lw["w13"].scales,
                                      *self.xq.triple(), *self.moe_dq.triple(),
                                      S, wts, ka)
            k.q40_gemv_grouped(lw["w2"].qs, lw["w2"].scales,
                               *self.moe_dq.triple(), self.moe_idx[:S],
                               self.moe_y, 1, router=wts, topk=ka, n_slots=S)
        else:
            wts, gate = self.moe_wts, {}
            k.moe_gate(self.moe_router[:NB], self.moe_idx, self.moe_wts, NB, ka)
            k.q40_gemv_grouped(lw["w13"].qs, lw["w13"].scales,
                               *self.xq.triple(), self.moe_idx[:S],
                               self.moe_out13, ka)
            self._swiglu_q80(self.moe_out13, S, self.moe_dq)
            k.q40_gemv_grouped(lw["w2"].qs, lw["w2"].scales,
                               *self.moe_dq.triple(), self.moe_idx[:S],
                               self.moe_y, 1)
        if not self.tp_path:
            k.scale_merge_add(self.x[:NB], self.moe_y, wts, self.ssq[slot],
                              NB, ka, **gate)
        else:
            k.scale_merge(self.partial[:NB], self.moe_y, wts, NB, ka, **gate)
            self._sync_partial(NB, slot)

    # ------------------------------------------------------------ engine API

    def forward(self, tokens: torch.Tensor, positions: torch.Tensor) -> torch.Tensor:
        """Engine-compatible forward. positions must be a contiguous range.

        When a decode graph is captured and B==1, this is a single hipGraph
        replay (the graph advances the device position itself)."""
        B = tokens.shape[0]
        assert B <= self.n_batches
        p0 = self._first_position(positions, B)
        self.tokens[:B].copy_(tokens.to(self.device), non_blocking=True)
        if B == 1:
            self._decode_step(p0)
        else:
            self._follow_wide_tier(
                p0 + B - 1, emit_q80=not (B >= 8 and self.prefill_bf16))
            g = None
            if B == self.n_batches:
                # full prefill chunks replay a captured graph (eager chunk
                # cost is host-launch-bound: ~400 python kernel launches);
                # where capture is unsupported they run eager, silently
                g = self.graphs.get(("prefill", self.skip_logits), lambda: (
                    lambda: self.forward_buffers(B), 1, None, None))
            self._step_at(B, p0, g)
        if self.tp_path:
            NBp = _pow2_batch(B)
            self.k.logits_concat(self.logits_full, self.logits_gather[NBp], B)
            return self.logits_full[:B]
        return self.logits0[:B]

    def _first_position(self, positions, B: int) -> int:
        """positions[0] of a single-sequence step of B rows, checked."""
        self._rows_only()
        p0 = int(positions[0])
        if p0 + B > self.cfg.seq_len:
            raise ValueError(
                f"position {p0}+{B} exceeds seq_len {self.cfg.seq_len} "
                "(rebuild with a larger --max-seq-len / seq_len)")
        return p0

    def _step_at(self, B: int, p0: int, graph=None):
        """One step of B rows at p0 outside the decode graph: eager
        launches, or a replay of a graph that was captured from them."""
        self.pos.fill_(p0)
        self._graph_pos = None  # the decode graph no longer owns the position
        if graph is not None:
            graph.replay()
        else:
            self.forward_buffers(B)

    def _follow_wide_tier(self, last_pos: int, emit_q80: bool):
        """S of a step outside the decode graph (a prompt chunk, an eager
        decode step) whose last row is at last_pos: S=1 while the wide tier
        holds there, so that a sequence computes the same alone, as rows and
        with or without the graph; above the tier the S that was set before
        it, as such steps always ran. Looked at on every step, so S=1 never
        outlives the tier; a step without Q80 output has no wide kernel and
        stays out of it."""
        wide = emit_q80 and self._pick_splits(last_pos) == 1
        if wide != (self.attn_splits == 1):
            self._set_attn_splits(1 if wide else self._splits_above)

    def _decode_step(self, p0: int) -> bool:
        """One B=1 step at p0: a replay of the decode graph, captured here at
        p0's K-split count if wanted and absent, else eager. True: it sampled."""
        key, g = ("decode", self.logprobs), None
        if self.graphs.allowed("decode", self._graph_wanted):
            sp = self._pick_splits(p0)
            if sp != self.attn_splits:
                self._set_attn_splits(sp)  # drops the graphs of the old count
            if p0 != self._graph_pos:
                # before a capture too: its warmups write the KV row of pos
                self.pos.fill_(p0)
            g = self.graphs.get(key, self._decode_plan, on_error=lambda e:
                                self._capture_failed("decode", e))
        if g is None:
            self._follow_wide_tier(p0, emit_q80=True)
            self._step_at(1, p0)
            return False
        g.replay()
        self._graph_pos = p0 + 1  # the graph's pos_inc advanced it
        return self.graphs.entries[key][1]

    def _capture_failed(self, what: str, e: Exception):
        if self.comm.rank == 0:
            print(f"⚠️  {what} graph capture failed ({e}); "
                  "running eager (slower)", file=sys.stderr)

    # ------------------------------------------------------------ sampling

    def last_logits(self) -> torch.Tensor:
        """The full-vocabulary logits row the last B=1 step left on device.
        TP: the gathered slices are contiguous in vocabulary order (see
        _logits), so the flat gather buffer is the row."""
        if self.tp_path:
            return self.logits_gather[1].view(-1)[: self.cfg.vocab_size]
        return self.logits0[0]

    def _sampler(self) -> DeviceSampler:
        """The sampler's scratch and launches, sharing sample_params and
        sample_out; built on first use (before a capture: the capture
        warmups launch the sampler)."""
        if self._dev_sampler is None:
            self._dev_sampler = DeviceSampler(
                self.cfg.vocab_size, self.device, params=self.sample_params,
                out=self.sample_out, k=self.k)
            self._step_host = torch.zeros(self.n_batches + 4, dtype=torch.int64)
            if self.device.type == "cuda":
                self._step_host = self._step_host.pin_memory()
        return self._dev_sampler

    def sample_row(self, row: torch.Tensor, coin, temperature: float,
                   topp: float):
        """Sample from any device f32 logits row, eagerly (first token after
        prefill, --no-graph). None: resample on the host with the same coin
        (Sampler.sample_with_coin)."""
        smp = self._sampler()
        if not self.logprobs:
            return smp.sample(row, coin, temperature, topp)
        smp.fill_params(smp.host_params, coin, temperature, topp)
        smp.params.copy_(smp.host_params, non_blocking=True)
        row = row.reshape(-1)
        smp.launch(row)
        self._launch_logprobs(row, self.sample_out[0:1], self._sample_io)
        return self._read_sample()

    def forward_sample(self, tokens: torch.Tensor, positions: torch.Tensor,
                       coin, temperature: float, topp: float):
        """One decode step and its sampled token: a replay of the decode
        graph captured with device_sampling (else the step, then the sampler
        launches). Only the token id and the parameters go to the device and
        {token, status} comes back; the logits stay in place (last_logits),
        so a None result can be resampled by the caller."""
        assert tokens.shape[0] == 1
        p0 = self._first_position(positions, 1)
        smp, NB = self._sampler(), self.n_batches
        self._step_host[0] = int(tokens[0])
        smp.fill_params(self._step_host[NB:].view(torch.float64), coin,
                        temperature, topp)
        # one staged copy for token and parameters; tokens[1:] are rewritten
        # too (zeros): a B=1 step reads tokens[0] only
        self._step_in.copy_(self._step_host, non_blocking=True)
        if not self._decode_step(p0):
            self._sample_last()
        return self._read_sample() if self.logprobs else smp.read()

    def _sample_last(self):
        """The sampler over the last B=1 step's row and, with set_logprobs,
        the log-probabilities of what it picked. No host value: capturable."""
        row = self.last_logits()
        self._sampler().launch(row)
        if self.logprobs:
            self._launch_logprobs(row, self.sample_out[0:1], self._sample_io)

    # ------------------------------------------------------------ logprobs

    def set_logprobs(self, on: bool) -> None:
        """Report token log-probabilities: every sampler launch is followed
        by logprob_rows (k = 20, the most a request can ask for, so one graph
        serves every request) on the token the sampler wrote, and the step's
        one copy back brings them along (last_logprobs, rows_logprobs). Off
        (the default) nothing is launched or copied beyond {token, status}.
        The captured graphs of both settings are kept (it is in their key)."""
        self.logprobs = bool(on)
        if on:
            self._logprob_scratch()

    def _logprob_scratch(self):
        """Stage A's per-chunk partials for n_batches rows; built on first
        use (before a capture)."""
        if self._lp_scratch is None:
            n = self.n_batches * int(self.k.logprob_chunks(self.cfg.vocab_size))
            self._lp_scratch = (
                torch.zeros(2 * n, device=self.device),          # max, sum-exp
                torch.zeros(LP_MAXK * n, dtype=torch.int64,
                            device=self.device))                 # chunk top keys
        return self._lp_scratch

    @staticmethod
    def _lp_views(io: torch.Tensor, rows: int):
        """The f32 [rows, 22] and i32 [rows, 20] blocks of a result buffer
        of rows * LP_WORDS int64 words (after the rows' {token, status})."""
        a, b = 2 * rows, (2 + LP_F32 // 2) * rows
        return (io[a:b].view(torch.float32).view(rows, LP_F32),
                io[b:].view(torch.int32).view(rows, LP_MAXK))

    def _launch_logprobs(self, logits, targets, io, k: int = LP_MAXK):
        """logprob_rows over `logits` ([V] or [B, V], any row stride) for
        the device targets, into the blocks of the result buffer `io`."""
        rows = io.numel() // LP_WORDS
        self.k.logprob_rows(logits, self.cfg.vocab_size, targets, k,
                            *self._logprob_scratch(), *self._lp_views(io, rows))

    def _read_sample(self):
        """forward_sample's one synchronising read with set_logprobs on:
        {token, status} and the log-probability blocks together."""
        self._lp_host = host = self._sample_io.cpu()
        token, status = host[:2].tolist()
        return None if status else token

    @staticmethod
    def _lp_entries(host: torch.Tensor, rows: int, B: int) -> list:
        lp, ids = HipTransformer._lp_views(host, rows)
        lp, ids = lp[:B].tolist(), ids[:B].tolist()
        return [(r[0], r[1], i, r[2:]) for r, i in zip(lp, ids)]

    def last_logprobs(self):
        """(lse, logprob, top_ids[20], top_logprobs[20]) of the token the
        last sample_row / forward_sample picked, from that step's copy.
        After a None result `logprob` belongs to a stale token: the caller's
        resampled token has logit - lse."""
        if self._lp_host is None:
            raise RuntimeError("no step has run with set_logprobs(True)")
        return self._lp_entries(self._lp_host, 1, 1)[0]

    def rows_logprobs(self, B: int) -> list:
        """last_logprobs for each of the B rows of the last
        forward_rows_sample."""
        if self._lp_rows_host is None:
            raise RuntimeError("no row step has run with set_logprobs(True)")
        return self._lp_entries(self._lp_rows_host, self.n_batches, B)

    def logprob_targets(self, logits: torch.Tensor, targets) -> list:
        """log-probability of targets[b] under row b of the device logits
        [B, V] (one of -1 gives -inf): the same kernels at k = 0, one copy
        of B floats back. The logits are not copied."""
        if logits.dim() == 1:
            logits = logits[None]
        NB, out = self.n_batches, []
        for i in range(0, logits.shape[0], NB):
            chunk = logits[i: i + NB]
            B = chunk.shape[0]
            t = torch.tensor([int(x) for x in targets[i: i + B]],
                             dtype=torch.int64).to(self.device)
            io = torch.zeros(B * LP_WORDS, dtype=torch.int64, device=self.device)
            self._launch_logprobs(chunk, t, io, k=0)
            out += self._lp_views(io, B)[0][:, 1].tolist()
        return out

    # ------------------------------------------------------------ pages

    def _rows_only(self):
        if self.page_map is not None:
            raise ValueError(
                "a paged model steps rows only (forward_rows); one sequence "
                "runs on the unpaged default")

    def _paged(self):
        if self.page_map is None:
            raise ValueError("the model has no paged KV cache (kv_pages=0)")
        return self.page_map

    def set_slot_pages(self, slot: int, pages, first: int = 0) -> None:
        """Paged model: map pool pages into the slot's page table from page
        index `first`. ValueError for an id outside 0..kv_pages-1. The
        device table follows before the next row step."""
        self._paged().set_slot_pages(slot, pages, first)

    def clear_slot(self, slot: int) -> None:
        """Paged model: unmap every page of the slot."""
        self._paged().clear_slot(slot)

    def _send_page_table(self):
        """Copy the table rows of the slots whose mapping changed, on the
        current stream: ordered after the steps already queued and before
        the next one, a replayed row graph included. Nothing to send in
        steady decode."""
        pm = self.page_map
        for slot in sorted(pm.dirty):
            self.page_table[slot].copy_(
                torch.tensor(pm.device_row(slot), dtype=torch.int32))
            self.page_table_sends += 1
        pm.dirty.clear()

    # ------------------------------------------------------------ row steps

    def _rows_buffers(self):
        """What the host sends per ragged step, in one allocation so a
        single small copy stages it: int64 words [tokens NB | per-row sampler
        f64 {coin, temperature, topp, unused} 4*NB | row table int32 [NB, 2]].
        The table is last: a step whose table the device already holds (a
        replayed graph advanced it) copies the prefix only. Built on first
        use, with its pinned host twin."""
        if self._rows_io is None:
            NB, dev = self.n_batches, self.device
            self._rows_io = io = torch.zeros(6 * NB, dtype=torch.int64, device=dev)
            self.row_tokens = io[:NB]
            self.row_params = io[NB:5 * NB].view(torch.float64).view(NB, 4)
            self.rows = io[5 * NB:].view(torch.int32).view(NB, 2)
            if self.page_map is not None:
                self.row_addr = KVAddr("_paged", self.rows, self.page_table,
                                       self.page_size)
            else:
                self.row_addr = KVAddr("_rows", self.rows)
            # [token, status] of every row, then (set_logprobs) the rows'
            # f32 [NB, 22] and i32 [NB, 20] blocks: one copy returns it all
            self._rows_out = torch.zeros(NB * LP_WORDS, dtype=torch.int64,
                                         device=dev)
            self.rows_sample_out = self._rows_out[:2 * NB].view(NB, 2)
            self._rows_host = torch.zeros(6 * NB, dtype=torch.int64)
            if dev.type == "cuda":
                self._rows_host = self._rows_host.pin_memory()
            self._rows_copied = None  # event: the last staging copy is done
            self._rows_dev = []       # the table rows the device holds
            self._row_samplers = []
        return self._rows_io

    def _row_sampler(self, b: int) -> DeviceSampler:
        """Row b's sampler: its parameters and result live in row b of
        row_params / rows_sample_out."""
        while len(self._row_samplers) <= b:
            i = len(self._row_samplers)
            self._row_samplers.append(DeviceSampler(
                self.cfg.vocab_size, self.device, params=self.row_params[i],
                out=self.rows_sample_out[i], k=self.k))
        return self._row_samplers[b]

    def rows_logits(self, B: int | None = None) -> torch.Tensor:
        """[B, vocab] logits the last row step left on device."""
        out = self.logits_full if self.tp_path else self.logits0
        return out[:B, : self.cfg.vocab_size]

    def _stage_rows(self, tokens, slots, positions, params=None):
        """Validate a ragged step and copy it to the device; returns
        (B, table, decode_only). params: per-row (coin, temperature, topp)."""
        from .rows import check_rows, is_decode_step
        c, NB = self.cfg, self.n_batches
        tokens, slots, positions = check_rows(
            tokens, slots, positions, self.n_slots, c.seq_len, NB)
        B = len(tokens)
        stride = c.seq_len  # word 0 of a table row: the slot's first cache row
        if self.page_map is not None:
            self.page_map.check(slots, positions)
            self._send_page_table()
            stride = self.page_map.pages_per_seq  # ... or its page table row
        self._rows_buffers()
        if self._rows_copied is not None:
            self._rows_copied.synchronize()  # the host twin is free again
        host = self._rows_host
        table = [(s * stride, p) for s, p in zip(slots, positions)]
        host[:NB] = 0
        host[:B] = torch.tensor(tokens, dtype=torch.int64)
        hp = host[NB:5 * NB].view(torch.float64).view(NB, 4)
        hp.zero_()  # temperature 0: a row nobody samples is an argmax
        if params is not None:
            hp[:B, :3] = torch.tensor(params, dtype=torch.float64)
        words = 5 * NB
        if self._rows_dev[:B] != table:
            ht = host[5 * NB:].view(torch.int32).view(NB, 2)
            ht.zero_()
            ht[:B] = torch.tensor(table, dtype=torch.int32)
            words = 6 * NB
            self._rows_dev = list(table)
        self._rows_io[:words].copy_(host[:words], non_blocking=True)
        if self.device.type == "cuda":
            self._rows_copied = torch.cuda.Event()
            self._rows_copied.record(torch.cuda.current_stream(self.device))
        return B, table, is_decode_step(slots)

    def _forward_rows_buffers(self, B: int):
        """One ragged step over row_tokens[:B] addressed by the row table.
        Everything stays on device: capturable."""
        self._forward_explicit(B, self.row_addr)

    def _rows_step_and_sample(self, B: int):
        self._forward_rows_buffers(B)
        logits = self.rows_logits(B)
        for b in range(B):
            self._row_sampler(b).launch(logits[b])
        if self.logprobs:
            # one pair of launches for all B rows, on the tokens just written
            self._launch_logprobs(logits, self.rows_sample_out[:, 0],
                                  self._rows_out)

    def _rows_plan(self, B: int):
        """B all-decode rows and their samplers; the tail advances the table."""
        self._row_sampler(B - 1)  # buffers exist before the capture
        return (lambda: self._rows_step_and_sample(B), 2,
                lambda: self.k.rows_advance(self.rows, B), None)

    def _run_rows(self, B: int, table, decode_only: bool, sample: bool):
        """The staged step: a replay of the B-row graph when every row is a
        decode row, else eager launches."""
        sp = self._pick_splits(max(p for _, p in table), rows=True)
        if sp != self.attn_splits:
            self._set_attn_splits(sp)  # drops the row graphs with the scratch
        g = decode_only and self.graphs.get(
            ("rows", B, self.logprobs), lambda: self._rows_plan(B),
            self.row_graphs, lambda e: self._capture_failed("row-step", e))
        if g:
            g.replay()
            # the graph's rows_advance moved every row on
            self._rows_dev[:B] = [(base, p + 1) for base, p in table]
        elif sample:
            self._rows_step_and_sample(B)
        else:
            self._forward_rows_buffers(B)

    def forward_rows(self, tokens, slots, positions) -> torch.Tensor:
        """One ragged step: row b feeds tokens[b] at positions[b] of the
        sequence in KV slot slots[b]; returns logits [B, vocab]. Rows may be
        decode rows of different sequences, prompt chunks (several rows of
        one slot at consecutive positions), or both. ValueError, before any
        launch, for a slot >= n_slots, a position >= seq_len, a repeated
        (slot, position) or more than n_batches rows; on a paged model also
        for a position in or above an unmapped page of its slot, and for a
        row that would write into a page several table entries name."""
        B, table, decode_only = self._stage_rows(tokens, slots, positions)
        self._run_rows(B, table, decode_only, sample=False)
        return self.rows_logits(B)

    def forward_rows_sample(self, tokens, slots, positions, coins,
                            temperatures, topps) -> list:
        """forward_rows with every row's token sampled on device from its
        own {coin, temperature, topp}: one token or None per row. None keeps
        forward_sample's contract: resample that row on the host with the
        same coin from rows_logits()."""
        params = [(0.0 if c is None else float(c), float(t), float(p))
                  for c, t, p in zip(coins, temperatures, topps)]
        if len(params) != len(tokens):
            raise ValueError("one coin, temperature and topp per row")
        B, table, decode_only = self._stage_rows(tokens, slots, positions,
                                                 params)
        self._run_rows(B, table, decode_only, sample=True)
        picked = self.rows_sample_out[:B]
        if self.logprobs:  # still one synchronising read: everything at once
            self._lp_rows_host = host = self._rows_out.cpu()
            picked = host[:2 * self.n_batches].view(-1, 2)[:B]
        return [None if status else token for token, status in picked.tolist()]

    # ------------------------------------------------------------ graphs

    def _pick_splits(self, pos: int, rows: bool = False) -> int:
        # S=1 below wide_thresh: with Q80 output that is the wide
        # single-launch kernel, one memory latency and an LDS merge instead
        # of split + combine. S=8 from there, S=16 past the threshold
        # (tools/attn_kv16_probe). The GQA-grouped split (DLLAMA_GQA_ATTN)
        # measured slower and is never auto-picked.
        # rows: a row step. The model's own default keeps its pinned launch
        # list (tests/golden/launch_trace_rows.json: S=8 at short positions)
        # and skips the wide tier; S=1 is never handed to the pair there.
        # set_wide_rows turns the tier on for row steps: BatchEngine calls
        # it.
        if not self.adaptive_thresh:
            return self.attn_splits
        if ((self.wide_rows or not rows)
                and pos < min(self.wide_thresh, self.adaptive_thresh)):
            return 1
        if pos < self.adaptive_thresh:
            return 8
        return 16 if pos < 2048 else 32  # S=32 at 4k ctx: +12.5% same-box

    def set_wide_rows(self, on: bool = True):
        """Let row steps take the wide tier as single-sequence steps do. A
        caller that serves sequences through forward_rows (BatchEngine) asks
        for it, so that a sequence generates the same alone and batched; the
        model's own default stays the pinned S=8 launch list."""
        self.wide_rows = on

    def _set_attn_splits(self, s: int):
        """Switch the flash-decode K-split count mid-stream (long-context
        adaptivity): resize the split scratch and drop every captured graph,
        which names it. Decode state (KV caches, device pos) is untouched."""
        self.attn_splits = s
        if s != 1:
            self._splits_above = s
        self._alloc_attn_scratch()
        self.graphs.clear()

    def _decode_plan(self):
        """The decode graph's plan; its note says whether it samples."""
        sample = bool(self.device_sampling)
        if sample:  # its buffers exist before anything is captured
            self._sampler()

        def step():
            self.forward_buffers(1)
            if sample:
                self._sample_last()

        return step, 2, lambda: self.k.pos_inc(self.pos, 1), sample

    def capture_decode_graph(self):
        """From now on a B=1 step is one replay of a hipGraph of the whole
        decode step: forward, with device_sampling the sampler, pos advance
        (the HIP analog of the reference's recorded Vulkan command buffers,
        nn-vulkan.cpp:1065-1118). Captures it, or raises and steps run eager."""
        self._rows_only()
        self._graph_wanted = True
        self.graphs.capture(("decode", self.logprobs), self._decode_plan)
        self._graph_pos = None  # device pos unknown until first fill

    # what the store holds for the set_logprobs setting in force, read-only
    # (the benchmark replays _graph itself; tests look at all three)
    @property
    def _graph(self):
        return self.graphs.get(("decode", self.logprobs))

    @property
    def _graph_samples(self) -> bool:
        return bool(self._graph and self.graphs.entries["decode", self.logprobs][1])

    @property
    def _row_graphs(self) -> dict:
        return {k[1]: e[0] for k, e in self.graphs.entries.items()
                if k[0] == "rows" and k[2] == self.logprobs}
