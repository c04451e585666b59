"""Buffers and launches of the on-device temperature/top-p sampler
(csrc/sampler.hip) for one vocabulary size.

The host `tokenizer.Sampler` stays the owner of the RNG: it draws the coin,
this class only carries {coin, temperature, topp} to the device and
{token, status} back. `HipTransformer` embeds one (its parameters living in
the model's per-step input buffer); tests and tools use it on its own.
"""

from __future__ import annotations

import torch

from . import hip_ops


class DeviceSampler:
    def __init__(self, vocab_size: int, device, params: torch.Tensor | None = None,
                 out: torch.Tensor | None = None, k=None):
        self.k = k = k or hip_ops()
        self.vocab_size = vocab_size
        dev = torch.device(device)
        # f64 {coin, temperature, topp, unused}: read by the kernels at run
        # time, so a captured graph follows per-request changes
        self.params = (torch.zeros(4, dtype=torch.float64, device=dev)
                       if params is None else params)
        self.out = (torch.zeros(2, dtype=torch.int64, device=dev)
                    if out is None else out)  # token, status
        nblk = int(k.sampler_blocks(vocab_size))
        self.scratch = (
            torch.zeros(2 * nblk, device=dev),                  # block max, sum-exp
            torch.zeros(nblk, dtype=torch.int64, device=dev),   # block argmax
            torch.zeros(nblk, device=dev),                      # block sums of p
            torch.zeros(int(k.sampler_max_candidates()),
                        dtype=torch.int64, device=dev),         # candidate sort keys
            torch.zeros(1, dtype=torch.int32, device=dev))      # candidate counter
        self.host_params = torch.zeros(4, dtype=torch.float64)
        if dev.type == "cuda":
            self.host_params = self.host_params.pin_memory()

    @staticmethod
    def fill_params(dst: torch.Tensor, coin, temperature: float, topp: float):
        dst[0] = 0.0 if coin is None else coin
        dst[1] = temperature
        dst[2] = topp

    def launch(self, row: torch.Tensor):
        """The three sampler kernels over an f32 logits row, parameters from
        `params`, result into `out`. No host value involved: capturable."""
        self.k.sample_logits(row, self.vocab_size, self.params, *self.scratch,
                             self.out)

    def read(self):
        """One 16-byte copy back (it also waits for the launches): the token,
        or None when more candidates passed the cutoff than the cap holds."""
        token, status = self.out.tolist()
        return None if status else token

    def sample(self, row: torch.Tensor, coin, temperature: float, topp: float):
        """Eager sample from any device f32 row; None = resample on the host
        with the same coin (`Sampler.sample_with_coin`)."""
        self.fill_params(self.host_params, coin, temperature, topp)
        self.params.copy_(self.host_params, non_blocking=True)
        self.launch(row.reshape(-1))
        return self.read()
