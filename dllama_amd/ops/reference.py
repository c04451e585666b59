"""PyTorch fp32 reference implementations of every op.

These define the numerics the HIP kernels are tested against (the same role
the f32 CPU kernels play for the quantized kernels in the reference's
nn-cpu-ops-test.cpp:126-277). They also power the CPU backend (BASELINE
config 1 runs without a GPU).

All activation tensors are fp32. Quantized-activation matmuls model the
Q80 round-trip explicitly so CPU and HIP paths see the same quantization
error profile.
"""

from __future__ import annotations

import torch

Q_BLOCK = 32


# ------------------------------------------------------------ quantize

def q80_quantize(x: torch.Tensor):
    """f32 [.., n] -> (q int8 [.., n], s f32 [.., n/32], bsum f32 [.., n/32]).

    d = absmax/127, q = round(x/d) (reference nn-quants.cpp quantizeF32toQ80);
    bsum = sum of the int8 values of the block (used by the GEMV to correct
    for the Q40 nibble offset of 8).
    """
    shape = x.shape
    g = x.reshape(*shape[:-1], shape[-1] // Q_BLOCK, Q_BLOCK).float()
    absmax = g.abs().amax(dim=-1)
    d = absmax / 127.0
    inv = torch.where(d > 0, 1.0 / torch.where(d == 0, torch.ones_like(d), d),
                      torch.zeros_like(d))
    q = torch.round(g * inv.unsqueeze(-1)).clamp(-127, 127).to(torch.int8)
    bsum = q.float().sum(dim=-1)
    return q.reshape(shape), d, bsum


def q80_dequantize(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    shape = q.shape
    g = q.reshape(*shape[:-1], shape[-1] // Q_BLOCK, Q_BLOCK).float()
    return (g * s.unsqueeze(-1)).reshape(shape)


def q80_roundtrip(x: torch.Tensor) -> torch.Tensor:
    q, s, _ = q80_quantize(x)
    return q80_dequantize(q, s)


def q80_quantize_f16(x: torch.Tensor):
    """f32 [.., n] -> (codes int8 [.., n], scales f16 [.., n/32]): Q80 blocks
    as they are stored (quants.quantize_q80, the Q80 KV cache). The codes
    come from the f32 scale d = absmax/127; the stored scale is f16(d)."""
    q, d, _ = q80_quantize(x)
    return q, d.to(torch.float16)


def q80_roundtrip_f16(x: torch.Tensor) -> torch.Tensor:
    """Round trip through stored Q80 blocks: code * f32(f16(d)). Equals
    quants.q80_roundtrip bit for bit; q80_roundtrip above keeps d in f32 (an
    activation cast, whose scale never leaves registers)."""
    q, s = q80_quantize_f16(x)
    return q80_dequantize(q, s.float())


# ------------------------------------------------------------ matmul

def q40_planes_dequant(qs: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """Device-layout Q40 planes -> f32 weight [d, n].

    qs uint8 [d, n/2] (block nibbles: byte j of block = elem j | elem j+16<<4),
    scales f16/f32 [d, n/32].
    """
    d, half = qs.shape
    n = half * 2
    nb = n // Q_BLOCK
    b = qs.reshape(d, nb, 16)
    lo = (b & 0xF).to(torch.int8) - 8
    hi = (b >> 4).to(torch.int8) - 8
    vals = torch.cat([lo, hi], dim=-1).float()  # [d, nb, 32]
    vals = vals * scales.float().unsqueeze(-1)
    return vals.reshape(d, n)


def q40_matmul(x: torch.Tensor, w_f32: torch.Tensor,
               quantize_x: bool = True) -> torch.Tensor:
    """y[B, d] = x[B, n] @ w[d, n]^T with the Q80 activation round-trip
    (reference matmul_Q80_Q40_F32, nn-cpu-ops.cpp:231-449)."""
    if quantize_x:
        x = q80_roundtrip(x)
    return x @ w_f32.t()


# ------------------------------------------------------------ exact oracle

def q40_unpack(qs: torch.Tensor) -> torch.Tensor:
    """Device-layout nibble plane uint8 [.., d, n/2] -> int64 [.., d, nb, 32]
    in -8..7: in block byte j the low nibble is element j, the high nibble
    element j+16."""
    half = qs.shape[-1]
    b = qs.cpu().reshape(*qs.shape[:-1], half // 16, 16).to(torch.int64)
    return torch.cat([(b & 0xF) - 8, (b >> 4) - 8], dim=-1)


def q40_q80_exact(qs, scales, xq, xs, blocks=None):
    """Exact Q40 x Q80 product: (y, A) float64 [B, d].

    qs uint8 [d, n/2] and scales f16/f32 [d, n/32] are the device-layout
    weight planes, xq int8 [B, n] and xs f32 [B, n/32] the Q80 codes and
    scales. Per block the integer dot is taken in int64, then
        t[b,row,j] = float64(scales[row,j]) * float64(xs[b,j]) * idot[b,row,j]
        y = sum_j t        A = sum_j |t|
    blocks=(j0, j1) restricts both sums to that block range (a K-split
    slice). The blocksum is not an input: the true value of the kernels'
    `idot_unsigned - 8*bsum` is the signed dot, so a wrong blocksum shows as
    an error of y. float64 holds every t exactly up to 2^-53, so y is good to
    about nb * 2^-53 * A."""
    w = q40_unpack(qs)                                   # [d, nb, 32]
    d, nb, _ = w.shape
    xq = xq.cpu()
    B = xq.shape[0]
    x = xq.reshape(B, nb, Q_BLOCK).to(torch.int64)
    j0, j1 = (0, nb) if blocks is None else blocks
    idot = torch.einsum("rjk,bjk->brj", w[:, j0:j1], x[:, j0:j1])
    sw = scales.cpu().to(torch.float64)[:, j0:j1]
    sx = xs.cpu().to(torch.float64)[:, j0:j1]
    t = sw.unsqueeze(0) * sx.unsqueeze(1) * idot.to(torch.float64)
    return t.sum(-1), t.abs().sum(-1)


def q40_q80_bound(nb: int, A):
    """Largest |f32 kernel output - q40_q80_exact y| of a correct kernel:
    (nb + 2) * 2^-24 * A, with u = 2^-24 the f32 unit roundoff.

    - The integer part is exact in f32. A kernel forms either the signed
      block dot (MFMA GEMM) or (float)idot_unsigned - 8*bsum (dot4 GEMV);
      |idot_unsigned| <= 32*15*127 = 60960 and |8*bsum| <= 8*32*127 = 32512,
      so both operands and their difference are integers below 2^24.
    - sw*sx rounds once: the kernel's term is t_j(1+e_j), |e_j| <= u.
    - Summing nb such terms in f32 in ANY order (fma or mul+add chain, lane
      partition, wave tree reduce, K-split partials and their reduction)
      errs by at most gamma_{nb-1} * sum|t_j(1+e_j)| with
      gamma_k = k*u/(1 - k*u); an fma folds the product's rounding into the
      add's, so it never does worse than this. Adding the zeros of idle
      lanes is exact.
    - Together: u*A + gamma_{nb-1}*(1+u)*A <= (nb + 2)*u*A for nb*u << 1
      (the margin of 2u*A absorbs the second-order terms up to nb ~ 2^23).
    A is the oracle's sum_j |t_j|. Derived, not tuned: a correct kernel over
    it means this derivation is wrong."""
    return (nb + 2) * 2.0 ** -24 * A


def q80_emit_check(codes, scales, bsum, v, v_tol, scale_rtol=0.0):
    """Assert that (codes int8 [.., n], scales [.., n/32], bsum [.., n/32])
    is a Q80 triple of values whose float64 truth is v [.., n] and that the
    emitting kernel saw with an error of at most v_tol (scalar or [.., n]).

    From q80_quant_lane (d = amax/127, code = rintf(x * (1/d))), per block:
      |code| <= 127
      bsum == sum(codes)                      exactly
      |d - max|v|/127| <= max(v_tol)/127 + 2^-22 * d
      |code*d - v| <= d/2 + v_tol + 127 * 2^-22 * d
    The kernel's amax is within max(v_tol) of max|v| and the divide rounds
    once (u*d). x*(1/d) carries the reciprocal's and the product's rounding,
    2u relative on a quotient of at most 127; rintf then adds at most 1/2,
    so |code - x/d| <= 1/2 + 127*2u. 2^-22 = 4u leaves room for divides
    that are good to 2 ulp instead of correctly rounded.

    The TP wire format stores f16(d) and no blocksum: pass bsum=None and
    scale_rtol=2^-11 (f16 half-ulp); the scale is then known to that
    relative error only, which adds scale_rtol*d to the scale check and
    127*scale_rtol*d to the code check."""
    codes = codes.cpu()
    n = codes.shape[-1]
    lead = codes.shape[:-1]
    c = codes.reshape(*lead, n // Q_BLOCK, Q_BLOCK).to(torch.float64)
    d = scales.cpu().to(torch.float64).reshape(*lead, n // Q_BLOCK)
    v = torch.as_tensor(v, dtype=torch.float64).reshape(c.shape)
    tol = torch.as_tensor(v_tol, dtype=torch.float64)
    tol = tol.expand(*lead, n).reshape(c.shape) if tol.dim() else tol.expand(c.shape)
    assert c.abs().max() <= 127, ("code out of range", c.abs().max().item())
    if bsum is not None:
        bs = bsum.cpu().to(torch.float64).reshape(*lead, n // Q_BLOCK)
        assert torch.equal(bs, c.sum(-1)), \
            ("blocksum != sum(codes)", (bs - c.sum(-1)).abs().max().item())
    eps4 = 2.0 ** -22 + scale_rtol
    d_err = (d - v.abs().amax(-1) / 127.0).abs()
    d_tol = tol.amax(-1) / 127.0 + eps4 * d
    assert (d_err <= d_tol).all(), ("scale", (d_err - d_tol).max().item())
    c_err = (c * d.unsqueeze(-1) - v).abs()
    c_tol = (d / 2 + 127 * eps4 * d).unsqueeze(-1) + tol
    assert (c_err <= c_tol).all(), ("code", (c_err - c_tol).max().item())


# ------------------------------------------------------------ norm / act

def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """y = w * x / sqrt(mean(x^2) + eps) over the last dim
    (reference invRms_F32 + rmsNorm_F32, nn-cpu-ops.cpp:114-175)."""
    inv = torch.rsqrt(x.float().pow(2).mean(dim=-1, keepdim=True) + eps)
    return x * inv * w


def silu(x: torch.Tensor) -> torch.Tensor:
    return x * torch.sigmoid(x)


def swiglu(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """silu(a) * b (reference OP_SILU + OP_MUL fusion)."""
    return silu(a) * b


def gelu(x: torch.Tensor) -> torch.Tensor:
    """tanh-approx GELU (reference gelu_F32, nn-cpu-ops.cpp:454-460)."""
    return 0.5 * x * (1.0 + torch.tanh(0.797884560802865 * (x + 0.044715 * x ** 3)))


# ------------------------------------------------------------ rope

def rope_cache(seq_len: int, head_dim: int, theta: float,
               scaling: dict | None = None) -> torch.Tensor:
    """cos/sin cache [seq_len, head_dim/2, 2].

    One head's worth serves every head on every rank: TP slices are whole
    heads, so (global dim % head_dim) == (local dim % head_dim)
    (cf. reference per-node cache, nn-core.cpp:326-383).
    scaling: llama3.1 frequency scaling dict(factor, low_freq_factor,
    high_freq_factor, orig_max_seq_len) (nn-core.cpp:326-340).
    """
    half = head_dim // 2
    j = torch.arange(half, dtype=torch.float32)
    freqs = 1.0 / theta ** (2.0 * j / head_dim)
    if scaling and scaling.get("factor", 1.0) != 1.0:
        freqs = _scale_freqs_llama3(freqs, scaling)
    pos = torch.arange(seq_len, dtype=torch.float32)
    ang = pos[:, None] * freqs[None, :]
    return torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1)


def _scale_freqs_llama3(freqs: torch.Tensor, s: dict) -> torch.Tensor:
    import math
    factor = s["factor"]
    lo_f = s["low_freq_factor"]
    hi_f = s["high_freq_factor"]
    orig = s["orig_max_seq_len"]
    wavelen = 2 * math.pi / freqs
    high_wl = orig / hi_f
    low_wl = orig / lo_f
    smooth = (orig / wavelen - lo_f) / (hi_f - lo_f)
    scaled = torch.where(wavelen < high_wl, freqs,
                         torch.where(wavelen > low_wl, freqs / factor,
                                     (1 - smooth) * freqs / factor + smooth * freqs))
    return scaled


def rope_llama(x: torch.Tensor, cache: torch.Tensor, positions: torch.Tensor,
               head_dim: int) -> torch.Tensor:
    """Interleaved-pair rotation (reference ropeLlama_F32,
    nn-cpu-ops.cpp:843-863). x [B, dim0] with dim0 a multiple of head_dim."""
    B, dim0 = x.shape
    xs = x.reshape(B, dim0 // head_dim, head_dim // 2, 2).float()
    c = cache[positions.long()]  # [B, hd/2, 2]
    cr, ci = c[..., 0].unsqueeze(1), c[..., 1].unsqueeze(1)
    x0, x1 = xs[..., 0], xs[..., 1]
    out = torch.stack([x0 * cr - x1 * ci, x0 * ci + x1 * cr], dim=-1)
    return out.reshape(B, dim0).to(x.dtype)


def rope_falcon(x: torch.Tensor, cache: torch.Tensor, positions: torch.Tensor,
                head_dim: int) -> torch.Tensor:
    """Half-rotated (NeoX) rotation (reference ropeFalcon_F32,
    nn-cpu-ops.cpp:865-885)."""
    B, dim0 = x.shape
    half = head_dim // 2
    xs = x.reshape(B, dim0 // head_dim, 2, half).float()  # [B,H,{lo,hi},half]
    c = cache[positions.long()]
    cr, ci = c[..., 0].unsqueeze(1), c[..., 1].unsqueeze(1)
    x0, x1 = xs[:, :, 0], xs[:, :, 1]
    out = torch.stack([x0 * cr - x1 * ci, x0 * ci + x1 * cr], dim=2)
    return out.reshape(B, dim0).to(x.dtype)


# ------------------------------------------------------------ attention

def attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
              positions: torch.Tensor, n_heads0: int, head_dim: int) -> torch.Tensor:
    """Causal decode/prefill attention over the KV cache
    (reference multiheadAtt_F32, nn-cpu-ops.cpp:753-788).

    q [B, n_heads0*head_dim]; k_cache/v_cache [seq, kv_dim0];
    positions [B] — row b attends to cache rows 0..positions[b].
    GQA: kv head = head // (n_heads0*head_dim // kv_dim0 ... ) computed from
    the head ratio.
    """
    B = q.shape[0]
    kv_dim0 = k_cache.shape[1]
    n_kv0 = kv_dim0 // head_dim
    kv_mul = n_heads0 // n_kv0
    scale = 1.0 / head_dim ** 0.5
    qh = q.reshape(B, n_heads0, head_dim).float()
    out = torch.empty_like(qh)
    for b in range(B):
        plen = int(positions[b].item()) + 1
        k = k_cache[:plen].reshape(plen, n_kv0, head_dim).float()
        v = v_cache[:plen].reshape(plen, n_kv0, head_dim).float()
        for h in range(n_heads0):
            kvh = h // kv_mul
            scores = (k[:, kvh] @ qh[b, h]) * scale
            probs = torch.softmax(scores, dim=0)
            out[b, h] = probs @ v[:, kvh]
    return out.reshape(B, n_heads0 * head_dim)


# ------------------------------------------------------------ moe

def moe_gate(router_logits: torch.Tensor, k: int, norm_topk: bool = True):
    """softmax -> top-k -> (normalized) weights
    (reference OP_SOFTMAX + OP_MOE_GATE, nn-cpu-ops.cpp:1443-1492)."""
    probs = torch.softmax(router_logits.float(), dim=-1)
    w, idx = torch.topk(probs, k, dim=-1)
    if norm_topk:
        w = w / w.sum(dim=-1, keepdim=True)
    return idx, w


# ------------------------------------------------------------ sync helpers

def q80_sync_pack(x: torch.Tensor) -> torch.Tensor:
    """Pack an f32 slice [B, n] into the Q80 wire layout used for the
    all-gather sync buffer: int8 payload then f16 scales, per batch row
    (role of reference cast-forward-f32-q80 + SYNC_NODE_SLICES)."""
    B, n = x.shape
    q, s, _ = q80_quantize(x)
    nb = n // Q_BLOCK
    out = torch.empty(B, n + 2 * nb, dtype=torch.uint8)
    out[:, :n] = q.view(torch.uint8)
    out[:, n:] = s.to(torch.float16).view(torch.uint8).reshape(B, 2 * nb)
    return out


def q80_sync_unpack(buf: torch.Tensor, n: int) -> torch.Tensor:
    """Inverse of q80_sync_pack -> f32 [B, n]."""
    B = buf.shape[0]
    nb = n // Q_BLOCK
    q = buf[:, :n].clone().view(torch.int8)
    s = buf[:, n:].contiguous().view(torch.float16).reshape(B, nb)
    return q80_dequantize(q, s.float())


# ------------------------------------------------------------ sampling

def sample_ref(logits, temperature: float, topp: float, coin: float):
    """float64 oracle of the sampler's selection rule (tokenizer.Sampler):
    returns (token, margin). margin is the smallest relative distance of any
    decision from flipping — |c_i - topp| over the candidate list and
    |c_i - r| / c[last] over the nucleus, |cdf_i - coin| in multinomial
    mode, inf for greedy — so a test can tell which draws are legitimately
    sensitive to the f32 summation order of an implementation."""
    import numpy as np
    if isinstance(logits, torch.Tensor):
        logits = logits.detach().cpu().numpy()
    x = np.asarray(logits, dtype=np.float64).reshape(-1)
    v = x.shape[0]
    if temperature == 0.0:
        return int(np.argmax(x)), float("inf")
    x = x / float(temperature)
    p = np.exp(x - x.max())
    p /= p.sum()
    if topp <= 0 or topp >= 1:
        cdf = np.cumsum(p)
        tok = min(int(np.searchsorted(cdf, coin, side="right")), v - 1)
        return tok, float(np.abs(cdf - coin).min())
    cutoff = (1.0 - topp) / (v - 1)
    idx = np.nonzero(p >= cutoff)[0]
    order = idx[np.argsort(-p[idx], kind="stable")]
    c = np.cumsum(p[order])
    last = min(int(np.searchsorted(c, topp, side="right")), len(order) - 1)
    r = coin * c[last]
    pick = min(int(np.searchsorted(c[: last + 1], r, side="right")), last)
    margin = min(float(np.abs(c - topp).min()),
                 float(np.abs(c[: last + 1] - r).min() / c[last]))
    return int(order[pick]), margin


# ------------------------------------------------------------ log-probabilities

LOGPROB_MAXK = 20


def logprob_rows_ref(logits, targets, k: int):
    """Oracle of the logprob_rows kernel, and the CPU path of everything that
    reports log-probabilities: per row of `logits` ([B, V] or [V]) returns
    (lse [B], logprob of targets[b] [B], top-k logprobs [B, 20] descending,
    top-k ids [B, 20]); float64 values, int64 ids.

    logprob(i) = logits[i] - logsumexp(logits), in float64 on the f32 values:
    the model's distribution at temperature 1. The order is that of a stable
    descending sort of the f32 values: lower index first on equal values,
    -0.0 equal to +0.0. A target outside [0, V) gives -inf; entries past
    min(k, V) are -inf and -1."""
    x32 = torch.as_tensor(logits).detach().cpu().float()
    if x32.dim() == 1:
        x32 = x32[None]
    B, V = x32.shape
    if not 0 <= k <= LOGPROB_MAXK:
        raise ValueError(f"k must be 0..{LOGPROB_MAXK} (got {k})")
    x = x32.double()
    lse = torch.logsumexp(x, dim=-1)
    t = torch.as_tensor(targets, dtype=torch.int64).reshape(-1).cpu()[:B]
    valid = (t >= 0) & (t < V)
    picked = x.gather(1, t.clamp(0, V - 1)[:, None])[:, 0] - lse
    target_lp = torch.where(valid, picked,
                            torch.full_like(picked, float("-inf")))
    top_lp = torch.full((B, LOGPROB_MAXK), float("-inf"), dtype=torch.float64)
    top_id = torch.full((B, LOGPROB_MAXK), -1, dtype=torch.int64)
    n = min(k, V)
    if n:
        order = torch.sort(x32, dim=-1, stable=True, descending=True).indices[:, :n]
        top_id[:, :n] = order
        top_lp[:, :n] = x.gather(1, order) - lse[:, None]
    return lse, target_lp, top_lp, top_id
