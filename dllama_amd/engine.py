"""Inference engine: prefill/decode orchestration, sampling, timing stats.

Mirrors the reference app loop (src/dllama.cpp:13-116): prompt evaluated in
batches of <= n_batches tokens through the same graph, then single-token
decode; reports eval/pred tokens-per-second the same way
(dllama.cpp:104-115).

Under TP every rank runs the engine in lockstep; logits are gathered on all
ranks and sampling is deterministic (same seed), so no extra token
broadcast is needed (replaces the reference LlmControlPacket root->worker
broadcast, app.cpp:197-230).

BatchEngine (beyond the reference, which serves one sequence) steps many
sequences together through a model's KV slots, one ragged forward_rows step
at a time; InferenceEngine stays the single-sequence path.
"""

from __future__ import annotations

import time
from dataclasses import dataclass, field

import torch

from .ops.reference import logprob_rows_ref
from .tokenizer import Sampler


@dataclass
class TokenLogprob:
    """A generated token's log-probability under the model's distribution at
    temperature 1 (before top-p, whatever the request samples with), and the
    most likely tokens at that step as (id, logprob), most likely first."""
    token: int
    logprob: float
    top: list = field(default_factory=list)


def _entry_from_logits(row: torch.Tensor, token: int, k: int) -> TokenLogprob:
    """The host path: the oracle on the logits row the sampler saw."""
    _, lp, top_lp, top_id = logprob_rows_ref(row.reshape(1, -1), [token], k)
    return TokenLogprob(token, float(lp[0]), list(zip(
        top_id[0, :k].tolist(), top_lp[0, :k].tolist())))


def _entry_from_device(result, token: int, sampled, row, k: int) -> TokenLogprob:
    """From the device's (lse, logprob, top_ids, top_logprobs) of a row.
    sampled None: the device sampler gave up and `token` was resampled on
    the host from `row`; its log-probability is logit - lse."""
    lse, lp, ids, lps = result
    if sampled is None:
        lp = float(row[token]) - lse
    return TokenLogprob(token, lp, [(i, v) for i, v in zip(ids[:k], lps[:k])
                                    if i >= 0])


@dataclass
class GenStats:
    prefill_tokens: int = 0
    prefill_time: float = 0.0
    decode_tokens: int = 0
    decode_time: float = 0.0
    # prompt tokens whose K/V came from shared prefix pages (BatchEngine on
    # a paged model); they were not stepped
    cached_tokens: int = 0
    # one TokenLogprob per generated token when the request asked for them
    logprobs: list | None = None

    @property
    def eval_tok_s(self) -> float:
        return self.prefill_tokens / self.prefill_time if self.prefill_time else 0.0

    @property
    def pred_tok_s(self) -> float:
        return self.decode_tokens / self.decode_time if self.decode_time else 0.0


class InferenceEngine:
    def __init__(self, model, tokenizer=None, sampler: Sampler | None = None,
                 n_batches: int = 32):
        self.model = model
        self.tokenizer = tokenizer
        self.sampler = sampler
        self.n_batches = n_batches
        self.pos = 0

    def reset(self, pos: int = 0) -> None:
        self.pos = pos

    def _sync_device(self):
        if getattr(self.model, "device", None) is not None:
            d = self.model.device
            if d.type == "cuda":
                torch.cuda.synchronize(d)

    def prefill(self, tokens: list[int], start_pos: int | None = None) -> torch.Tensor:
        """Feed prompt tokens in chunks of n_batches; returns logits of the
        last token [vocab]."""
        if start_pos is not None:
            self.pos = start_pos
        logits = None
        starts = list(range(0, len(tokens), self.n_batches))
        for i in starts:
            chunk = tokens[i: i + self.n_batches]
            t = torch.tensor(chunk, dtype=torch.int64)
            p = torch.arange(self.pos, self.pos + len(chunk), dtype=torch.int64)
            # intermediate prefill chunks don't need logits (the reference
            # computes them anyway; real serving shouldn't)
            self.model.skip_logits = i != starts[-1]
            try:
                logits = self.model.forward(t, p)
            finally:
                self.model.skip_logits = False
            self.pos += len(chunk)
        return logits[-1]

    def decode_one(self, token: int) -> torch.Tensor:
        """One decode step; returns logits [vocab] for the next token."""
        t = torch.tensor([token], dtype=torch.int64)
        p = torch.tensor([self.pos], dtype=torch.int64)
        logits = self.model.forward(t, p)
        self.pos += 1
        return logits[0]

    def _device_sampling(self) -> bool:
        """The model samples on device (HipTransformer with device_sampling):
        it offers sample_row and forward_sample and has not switched them
        off. Any other model keeps the host sampling path."""
        m = self.model
        return (hasattr(m, "sample_row") and hasattr(m, "forward_sample")
                and bool(getattr(m, "device_sampling", True)))

    @staticmethod
    def _coin(sampler: Sampler) -> float:
        """The host Sampler owns the RNG: one draw per sampled token, none at
        temperature 0 — the same stream as Sampler.sample."""
        return sampler.next_coin() if sampler.temperature != 0.0 else 0.0

    def decode_sample(self, token: int, sampler: Sampler,
                      logprobs: int | None = None):
        """One decode step with the token sampled on device. When the device
        sampler gives up (more candidates than its cap) the logits it left in
        place are resampled on the host path with the same coin. With
        logprobs (the model's set_logprobs is on) returns (token, entry)."""
        t = torch.tensor([token], dtype=torch.int64)
        p = torch.tensor([self.pos], dtype=torch.int64)
        coin = self._coin(sampler)
        nxt = sampled = self.model.forward_sample(t, p, coin, sampler.temperature,
                                                  sampler.topp)
        self.pos += 1
        if nxt is None:
            nxt = sampler.sample_with_coin(self.model.last_logits(), coin)
        if logprobs is None:
            return nxt
        return nxt, _entry_from_device(self.model.last_logprobs(), nxt, sampled,
                                       self.model.last_logits(), logprobs)

    def generate(self, prompt_tokens: list[int], max_tokens: int,
                 on_token=None, stop_check=None, logprobs: int | None = None,
                 on_logprobs=None) -> tuple[list[int], GenStats]:
        """Greedy/sampled generation. on_token(token_id) is called per new
        token; stop_check(token_id) -> bool ends generation. logprobs = K
        (0..20): stats.logprobs gets one TokenLogprob per generated token
        with its K most likely alternatives, and on_logprobs(entry) is called
        right after on_token. The tokens do not depend on it."""
        if logprobs is None:
            return self._generate(prompt_tokens, max_tokens, on_token,
                                  stop_check, None, None)
        if not 0 <= logprobs <= 20:
            raise ValueError(f"logprobs must be 0..20 (got {logprobs})")
        switch = (self._device_sampling()
                  and hasattr(self.model, "set_logprobs"))
        if switch:
            self.model.set_logprobs(True)
        try:
            return self._generate(prompt_tokens, max_tokens, on_token,
                                  stop_check, logprobs, on_logprobs)
        finally:
            if switch:
                self.model.set_logprobs(False)

    def _generate(self, prompt_tokens, max_tokens, on_token, stop_check,
                  logprobs, on_logprobs):
        stats = GenStats()
        assert len(prompt_tokens) >= 1

        self._sync_device()
        t0 = time.perf_counter()
        logits = self.prefill(prompt_tokens)
        self._sync_device()
        stats.prefill_time = time.perf_counter() - t0
        stats.prefill_tokens = len(prompt_tokens)

        out: list[int] = []
        sampler = self.sampler or Sampler(logits.shape[-1], 0.0, 0.9, 12345)
        on_device = self._device_sampling()
        lp_device = on_device and hasattr(self.model, "set_logprobs")
        if logprobs is not None:
            stats.logprobs = []

        def emit(token, entry):
            out.append(token)
            if on_token:
                on_token(token)
            if logprobs is not None:
                stats.logprobs.append(entry)
                if on_logprobs:
                    on_logprobs(entry)

        t0 = time.perf_counter()
        entry = None
        if on_device:
            coin = self._coin(sampler)
            token = sampled = self.model.sample_row(
                logits, coin, sampler.temperature, sampler.topp)
            if token is None:
                token = sampler.sample_with_coin(logits, coin)
            if logprobs is not None and lp_device:
                entry = _entry_from_device(self.model.last_logprobs(), token,
                                           sampled, logits, logprobs)
        else:
            token = sampler.sample(logits)
        if logprobs is not None and entry is None:
            entry = _entry_from_logits(logits, token, logprobs)
        emit(token, entry)
        seq_len = getattr(getattr(self.model, "cfg", None), "seq_len", None)
        for _ in range(max_tokens - 1):
            if stop_check and stop_check(token):
                break
            if seq_len is not None and self.pos >= seq_len:
                break  # context window exhausted (reference clamps via seqLen)
            entry = None
            if on_device and logprobs is not None and lp_device:
                token, entry = self.decode_sample(token, sampler, logprobs)
            elif on_device:
                token = self.decode_sample(token, sampler)
                if logprobs is not None:
                    entry = _entry_from_logits(self.model.last_logits(), token,
                                               logprobs)
            else:
                logits = self.decode_one(token)
                token = sampler.sample(logits)
                if logprobs is not None:
                    entry = _entry_from_logits(logits, token, logprobs)
            emit(token, entry)
        self._sync_device()
        stats.decode_time = time.perf_counter() - t0
        stats.decode_tokens = len(out)
        return out, stats


class _Sequence:
    """One submitted request of a BatchEngine."""

    def __init__(self, prompt, max_tokens, sampler, on_token, stop_check,
                 logprobs=None, on_logprobs=None):
        self.logprobs = logprobs
        self.on_logprobs = on_logprobs
        self.prompt = list(prompt)
        self.max_tokens = max_tokens
        self.sampler = sampler
        self.on_token = on_token
        self.stop_check = stop_check
        self.slot = None      # KV slot while running
        self.fed = 0          # prompt tokens already stepped (or shared)
        self.pages = []       # paged model: pool pages held, by page index
        self.registered = 0   # ... of which the first so many are indexed
        self.written = 0      # positions whose K/V the slot holds
        self.out: list[int] = []
        self.done = False
        self.stats = GenStats(prefill_tokens=len(self.prompt),
                              logprobs=None if logprobs is None else [])
        self._t0 = None       # when first scheduled, then when first sampled

    @property
    def tokens(self) -> list[int]:
        return self.out

    @property
    def prefilling(self) -> bool:
        return self.fed < len(self.prompt)


class BatchEngine:
    """Many sequences through one model, one ragged step at a time.

    The model (HipTransformer or CpuTransformer, built with n_slots slots)
    offers forward_rows; every running sequence owns one of its KV slots.
    step() builds one step of at most n_batches rows: first one decode row
    for every running sequence, then prompt chunks of the sequences that are
    still prefilling, in submission order. Sequences beyond the slot count
    wait; a finished sequence frees its slot for the next. Each sequence
    owns its Sampler (its own RNG stream), so what it generates does not
    depend on what it is batched with.

    On a paged model (kv_pages > 0) a sequence also needs pages: admission
    is FIFO and takes a free slot plus every page the sequence can come to
    use, reserved up front, so nothing runs out mid-flight and nothing is
    preempted. If the head of the queue does not fit it waits, and nothing
    overtakes it. With share_prefixes the leading full pages of a prompt
    that are cached in the pool's prefix index are mapped instead of
    computed (stats.cached_tokens), and every page a sequence fills, prompt
    or generated, is registered for later requests."""

    def __init__(self, model, tokenizer=None, n_batches: int = 32,
                 share_prefixes: bool = True):
        if not hasattr(model, "forward_rows"):
            raise ValueError("BatchEngine needs a model with forward_rows")
        self.model = model
        self.pool = None
        if getattr(model, "page_map", None) is not None:
            from .models.pages import PagePool
            self.pool = PagePool(model.kv_pages, model.page_size,
                                 share=share_prefixes)
            for slot in range(model.n_slots):
                model.clear_slot(slot)
        # short-context row steps take the wide single-launch attention that
        # the single-sequence decode takes, so a sequence generates the same
        # alone and batched
        if hasattr(model, "set_wide_rows"):
            model.set_wide_rows()
        self.tokenizer = tokenizer
        self.n_batches = min(n_batches, getattr(model, "n_batches", n_batches))
        self.seq_len = model.cfg.seq_len
        self.free_slots = list(range(model.n_slots))
        self.waiting: list[_Sequence] = []
        self.running: list[_Sequence] = []
        self.last_step_rows: list[tuple] = []  # (sequence, position) per row

    _coin = staticmethod(InferenceEngine._coin)

    def _on_device(self) -> bool:
        """The model samples rows on device (HipTransformer with
        device_sampling); any other model samples on the host."""
        return (hasattr(self.model, "forward_rows_sample")
                and bool(getattr(self.model, "device_sampling", False)))

    def submit(self, prompt_tokens: list[int], max_tokens: int,
               sampler: Sampler | None = None, on_token=None,
               stop_check=None, logprobs: int | None = None,
               on_logprobs=None) -> _Sequence:
        """Queue a request; the handle's .tokens grows as it generates and
        .done turns True when it ended (max_tokens, stop_check or the end
        of the context window), .stats holding its timing. logprobs = K
        (0..20): .stats.logprobs gets one TokenLogprob per generated token
        and on_logprobs(entry) is called right after on_token."""
        if logprobs is not None and not 0 <= logprobs <= 20:
            raise ValueError(f"logprobs must be 0..20 (got {logprobs})")
        if len(prompt_tokens) < 1:
            raise ValueError("empty prompt")
        if len(prompt_tokens) > self.seq_len:
            raise ValueError(
                f"prompt of {len(prompt_tokens)} tokens exceeds seq_len "
                f"{self.seq_len} (rebuild with a larger --max-seq-len / seq_len)")
        if self.pool is not None:
            need = self._pages_needed(len(prompt_tokens), max_tokens)
            if need > self.pool.n_pages:
                raise ValueError(
                    f"a request of {len(prompt_tokens)} prompt tokens and "
                    f"max_tokens {max_tokens} needs {need} KV pages, the pool "
                    f"has {self.pool.n_pages} (raise --kv-pages / kv_pages)")
        if sampler is None:
            sampler = Sampler(self.model.cfg.vocab_size, 0.0, 0.9, 12345)
        seq = _Sequence(prompt_tokens, max_tokens, sampler, on_token,
                        stop_check, logprobs, on_logprobs)
        self.waiting.append(seq)
        return seq

    @property
    def idle(self) -> bool:
        return not self.waiting and not self.running

    def _pages_needed(self, n_prompt: int, max_tokens: int) -> int:
        P = self.pool.page_size
        return -(-min(n_prompt + max_tokens, self.seq_len) // P)

    def _take_pages(self, seq: _Sequence) -> bool:
        """Reserve the pages of the sequence's whole life: the cached
        pages of its prompt's prefix, shared, plus new ones. False, with
        nothing taken, when the pool cannot supply them now."""
        pool = self.pool
        shared = pool.match(seq.prompt)
        need = self._pages_needed(len(seq.prompt), seq.max_tokens)
        new = pool.alloc(need - len(shared))
        if new is None:
            pool.release(shared)
            return False
        seq.pages = shared + new
        seq.registered = len(shared)
        seq.fed = seq.written = len(shared) * pool.page_size
        seq.stats.cached_tokens = seq.fed
        return True

    def _register_pages(self, seq: _Sequence) -> None:
        """Index the pages the sequence has filled since the last step."""
        P = self.pool.page_size
        while (seq.registered + 1) * P <= seq.written:
            n = (seq.registered + 1) * P
            fed = seq.prompt[:n]
            fed += seq.out[: n - len(fed)]
            self.pool.register(fed, seq.pages[seq.registered])
            seq.registered += 1

    def _plan(self):
        """Rows of the next step as (sequence, token, position, samples)."""
        while self.waiting and self.free_slots:
            seq = self.waiting[0]
            if self.pool is not None and not self._take_pages(seq):
                break  # the head waits for pages; nothing overtakes it
            self.waiting.pop(0)
            seq.slot = self.free_slots.pop(0)
            if self.pool is not None:
                self.model.set_slot_pages(seq.slot, seq.pages)
            self.running.append(seq)
        rows = []
        for seq in self.running:
            if not seq.prefilling:
                pos = len(seq.prompt) + len(seq.out) - 1
                rows.append((seq, seq.out[-1], pos, True))
        for seq in self.running:
            room = self.n_batches - len(rows)
            if room <= 0:
                break
            if seq.prefilling:
                chunk = seq.prompt[seq.fed: seq.fed + room]
                last = seq.fed + len(chunk) == len(seq.prompt)
                for i, tok in enumerate(chunk):
                    rows.append((seq, tok, seq.fed + i,
                                 last and i == len(chunk) - 1))
        return rows

    def step(self) -> None:
        """Run one ragged step and hand every sampled token to its
        sequence."""
        rows = self._plan()
        if not rows:
            return
        now = time.perf_counter()
        for seq, _, _, _ in rows:
            if seq._t0 is None:
                seq._t0 = now
        self.last_step_rows = [(seq, pos) for seq, _, pos, _ in rows]
        tokens = [tok for _, tok, _, _ in rows]
        slots = [seq.slot for seq, _, _, _ in rows]
        positions = [pos for _, _, pos, _ in rows]
        model = self.model
        # the model computes log-probabilities while any running sequence
        # asks for them, and only the asking rows are turned into entries
        asking = any(seq.logprobs is not None for seq in self.running)
        lp_device = self._on_device() and hasattr(model, "set_logprobs")
        if lp_device:
            model.set_logprobs(asking)
        entries = [None] * len(rows)
        if self._on_device():
            coins = [self._coin(seq.sampler) if smp else 0.0
                     for seq, _, _, smp in rows]
            temps = [seq.sampler.temperature if smp else 0.0
                     for seq, _, _, smp in rows]
            topps = [seq.sampler.topp for seq, _, _, _ in rows]
            picked = model.forward_rows_sample(tokens, slots, positions, coins,
                                               temps, topps)
            logits = None
            sampled = list(picked)
            for b, (seq, _, _, smp) in enumerate(rows):
                if smp and picked[b] is None:
                    if logits is None:
                        logits = model.rows_logits(len(rows))
                    picked[b] = seq.sampler.sample_with_coin(logits[b], coins[b])
            if asking:
                if lp_device:
                    results = model.rows_logprobs(len(rows))
                elif logits is None:
                    logits = model.rows_logits(len(rows))
                for b, (seq, _, _, smp) in enumerate(rows):
                    if not smp or seq.logprobs is None:
                        continue
                    if lp_device:
                        entries[b] = _entry_from_device(
                            results[b], int(picked[b]), sampled[b],
                            None if sampled[b] is not None else logits[b],
                            seq.logprobs)
                    else:
                        entries[b] = _entry_from_logits(
                            logits[b], int(picked[b]), seq.logprobs)
        else:
            logits = model.forward_rows(tokens, slots, positions)
            picked = [seq.sampler.sample(logits[b]) if smp else None
                      for b, (seq, _, _, smp) in enumerate(rows)]
            for b, (seq, _, _, smp) in enumerate(rows):
                if smp and seq.logprobs is not None:
                    entries[b] = _entry_from_logits(logits[b], int(picked[b]),
                                                    seq.logprobs)
        now = time.perf_counter()
        for seq, _, pos, _ in rows:
            if seq.prefilling:
                seq.fed += 1
            seq.written = pos + 1  # a sequence's rows are in position order
        if self.pool is not None:
            for seq in self.running:
                self._register_pages(seq)
        for b, (seq, _, pos, smp) in enumerate(rows):
            if smp:
                self._accept(seq, int(picked[b]), now, entries[b])
        if lp_device and asking and not any(seq.logprobs is not None
                                            for seq in self.running):
            model.set_logprobs(False)  # the last asking sequence has ended

    def _accept(self, seq: _Sequence, token: int, now: float,
                entry: TokenLogprob | None = None) -> None:
        if not seq.out:
            seq.stats.prefill_time = now - seq._t0
            seq._t0 = now  # decode time runs from the first token on
        seq.out.append(token)
        if seq.on_token:
            seq.on_token(token)
        if entry is not None:
            seq.stats.logprobs.append(entry)
            if seq.on_logprobs:
                seq.on_logprobs(entry)
        # the same three ends as InferenceEngine.generate, in its order
        next_pos = len(seq.prompt) + len(seq.out) - 1
        if (len(seq.out) >= seq.max_tokens
                or (seq.stop_check and seq.stop_check(token))
                or next_pos >= self.seq_len):
            seq.done = True
            seq.stats.decode_tokens = len(seq.out)
            seq.stats.decode_time = now - seq._t0
            self.running.remove(seq)
            if self.pool is not None:
                self.pool.release(seq.pages)
                self.model.clear_slot(seq.slot)
                seq.pages = []
            self.free_slots.append(seq.slot)
            self.free_slots.sort()
            seq.slot = None

    def run(self) -> None:
        """Step until every submitted sequence has ended."""
        while not self.idle:
            self.step()

    def generate_many(self, prompts: list[list[int]], max_tokens: int,
                      samplers: list | None = None, on_token=None,
                      stop_check=None) -> list[tuple[list[int], GenStats]]:
        """Generate for every prompt; results in input order. samplers: one
        Sampler per prompt (default greedy); on_token(index, token) and
        stop_check(index, token) get the prompt's index first."""
        seqs = []
        for i, prompt in enumerate(prompts):
            seqs.append(self.submit(
                prompt, max_tokens, samplers[i] if samplers else None,
                (lambda t, i=i: on_token(i, t)) if on_token else None,
                (lambda t, i=i: stop_check(i, t)) if stop_check else None))
        self.run()
        return [(s.out, s.stats) for s in seqs]


def _to_numpy(x: torch.Tensor):
    return x.detach().float().cpu().numpy()
