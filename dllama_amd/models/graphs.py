"""A model's captured step graphs: one store, one capture, one invalidation.

A graph is valid for what its key names, at the `attn_splits` it was
captured at (its launches name the split scratch; a change: `clear()`):
    ("decode", logprobs)      the B=1 step; its note: it ends in the sampler
    ("prefill", skip_logits)  a full prompt chunk
    ("rows", B, logprobs)     an all-decode row step of B rows
A step comes as a plan: a callable that creates the buffers the step needs
and returns `(body, warmups, tail, note)`. The store holds no tensors.
"""

import torch


def capture_hip_graph(device, body, warmups: int, tail=None):
    """Synchronise, run body() `warmups` times on a side stream (allocations,
    lazy kernel loads), join and synchronise, then capture body() and tail()
    as a hipGraph. The tail (a position advance) never runs while warming
    up. Buffers that body() would create exist before this is called."""
    torch.cuda.synchronize(device)
    s = torch.cuda.Stream(device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        for _ in range(warmups):
            body()
    torch.cuda.current_stream(device).wait_stream(s)
    torch.cuda.synchronize(device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
        if tail is not None:
            tail()
    return g


class StepGraphs:
    def __init__(self, capture, on_gpu: bool):
        self._capture = capture  # (body, warmups, tail) -> has .replay()
        self.on_gpu = on_gpu     # there is a device to capture on
        # key -> (graph, note), and the kinds (key[0]) whose capture failed:
        # eager from then on, also after a clear(). A tool adds a kind to
        # run it eager everywhere.
        self.entries, self.failed = {}, set()

    def allowed(self, kind: str, enabled: bool = True) -> bool:
        """May a graph of this kind be captured (`enabled`: says the model)?"""
        return bool(enabled) and self.on_gpu and kind not in self.failed

    def get(self, key, plan=None, enabled=True, on_error=lambda e: None):
        """The graph for key, captured from plan if absent and allowed; else
        None: run eager. A failing capture goes to on_error, not the caller."""
        if key in self.entries and key[0] not in self.failed:
            return self.entries[key][0]
        if plan is None or not self.allowed(key[0], enabled):
            return None
        try:
            return self.capture(key, plan)
        except Exception as e:  # noqa: BLE001
            return on_error(e)

    def capture(self, key, plan):
        """Capture plan as key's graph; a failure is remembered, then raised."""
        try:
            body, warmups, tail, note = plan()
            self.entries[key] = (self._capture(body, warmups, tail), note)
        except Exception:
            self.failed.add(key[0])
            raise
        return self.entries[key][0]

    def clear(self) -> None:
        """Drop every graph: the split scratch they name is gone."""
        self.entries.clear()
