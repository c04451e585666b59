"""`dllama-api` — OpenAI-compatible HTTP server.

Behavior parity with the reference API server (src/dllama-api.cpp):
  - POST /v1/chat/completions (stream SSE + non-stream), GET /v1/models
    (routes, dllama-api.cpp:550-561)
  - params: stream / temperature / seed / max_tokens / stop
    (dllama-api.cpp:491-520)
  - NaiveCache: longest-prefix chat-history KV reuse by message-list
    comparison (dllama-api.cpp:298-343)
  - single-slot sequential serving over a stdlib HTTP server (the reference
    hand-rolls HTTP/1.1 the same way, dllama-api.cpp:45-186)
  - --slots N > 1 (one GPU): a threading server whose handlers enqueue
    requests to one scheduler thread; it owns the model and a BatchEngine
    and decodes up to N requests per step. Each request prefills from 0
    there (no NaiveCache reuse across slots) unless --kv-pages M pages the
    KV cache: then whole pages of a shared prompt prefix or chat history
    are reused across slots (usage.prompt_tokens_details.cached_tokens).
  - logprobs / top_logprobs (beyond the reference): per generated token its
    log-probability and the top_logprobs most likely tokens, under the
    model's distribution at temperature 1 ("raw logprobs"). Not under
    tensor parallelism; no prompt-token logprobs (echo).
"""

from __future__ import annotations

import json
import queue
import sys
import threading
import time
import uuid
from http.server import BaseHTTPRequestHandler, HTTPServer, ThreadingHTTPServer

from ..engine import BatchEngine
from ..tokenizer import Sampler

from ..tokenizer import (ChatItem, ChatTemplateGenerator, EosDetector,
                         EOS, MAYBE_EOS, TEMPLATE_UNKNOWN, chat_stops)
from .main import build_parser, load_engine


class NaiveCache:
    """Reuse the KV cache for the longest shared chat-message prefix
    (reference NaiveCache, dllama-api.cpp:298-343)."""

    def __init__(self):
        self.tokens: list[int] = []

    def resolve(self, new_tokens: list[int]) -> int:
        """-> start_pos: length of the shared prefix with the cached run."""
        n = 0
        for a, b in zip(self.tokens, new_tokens):
            if a != b:
                break
            n += 1
        # never reuse the full prompt (need at least 1 token to evaluate)
        n = min(n, len(new_tokens) - 1)
        return max(n, 0)

    def update(self, tokens: list[int]) -> None:
        self.tokens = list(tokens)


class BadRequest(ValueError):
    """A request the server answers with a 400; `param` names the field."""

    def __init__(self, message: str, param: str | None = None):
        super().__init__(message)
        self.param = param


def logprobs_requested(body: dict, world: int = 1) -> int | None:
    """K of a request's logprobs / top_logprobs fields (None: not asked
    for); BadRequest for what the API refuses."""
    want, top = body.get("logprobs"), body.get("top_logprobs")
    if want is not None and not isinstance(want, bool):
        raise BadRequest("logprobs must be a boolean", "logprobs")
    if top is not None:
        if isinstance(top, bool) or not isinstance(top, int) or not 0 <= top <= 20:
            raise BadRequest("top_logprobs must be an integer between 0 and 20",
                             "top_logprobs")
        if not want:
            raise BadRequest("top_logprobs requires logprobs to be true",
                             "top_logprobs")
    if not want:
        return None
    if world > 1:
        raise BadRequest("logprobs is not supported under tensor parallelism",
                         "logprobs")
    return top or 0


class _Deltas:
    """One request's way from tokens to text deltas: the streaming decoder
    feeds the EosDetector, and what it releases goes to emit(delta). With
    logprobs, emit(delta, entries) also gets the entries of the tokens whose
    text that delta released: tokens the detector held back go with the
    delta that releases them, and the token that ended the generation (an
    EOS id, or the one that completed a stop string) is not listed."""

    def __init__(self, tok, detector, emit, logprobs: bool):
        self.tok, self.detector, self.emit = tok, detector, emit
        self.logprobs = logprobs
        self.text: list[str] = []
        self.pending: list[dict] = []
        self.kind = None

    def on_token(self, t):
        # streaming-decoder first: UTF-8-safe pieces into the detector
        self.kind = self.detector.append(t, self.tok.decode(t))
        if not self.logprobs:
            self._release()

    def on_logprobs(self, entry):  # called right after on_token
        if self.kind != EOS:
            self.pending.append(self._json(entry))
        self._release()

    def _release(self):
        if self.kind == MAYBE_EOS:
            return
        delta = self.detector.get_delta()
        if delta:
            self.text.append(delta)
            self._emit(delta)
            self.detector.reset()
        elif self.pending:
            self._emit("")

    def finish(self):
        """Entries still held when the generation ended (max_tokens with a
        possible stop string pending): their text is never released."""
        if self.pending:
            self._emit("")

    def _emit(self, delta):
        if self.logprobs:
            entries, self.pending = self.pending, []
            self.emit(delta, entries)
        else:
            self.emit(delta)

    def _piece(self, token: int, logprob: float) -> dict:
        raw = self.tok.vocab[token] if 0 <= token < len(self.tok.vocab) else b""
        return {"token": raw.decode("utf-8", errors="replace"),
                # JSON has no infinity
                "logprob": logprob if logprob > -9999.0 else -9999.0,
                "bytes": list(raw)}

    def _json(self, entry) -> dict:
        out = self._piece(entry.token, entry.logprob)
        out["top_logprobs"] = [self._piece(i, lp) for i, lp in entry.top]
        return out


class BatchScheduler:
    """The one thread that owns the model in multi-slot serving. Handlers
    hand it requests over a queue; it admits them into a BatchEngine between
    steps, and every request's tokens flow back through the callbacks the
    request was submitted with (called on this thread)."""

    def __init__(self, model, tokenizer, n_batches: int):
        self.engine = BatchEngine(model, tokenizer, n_batches)
        self.inbox: queue.Queue = queue.Queue()
        self.active = []  # (sequence, on_done)
        self.thread = threading.Thread(target=self._loop, daemon=True)
        self.thread.start()

    def submit(self, tokens, max_tokens, sampler, on_token, stop_check, on_done,
               stats_out=None, logprobs=None, on_logprobs=None):
        """on_done(error_or_None) is called once, after the last on_token.
        stats_out: a list that receives the sequence's GenStats when it is
        queued in the engine."""
        self.inbox.put((tokens, max_tokens, sampler, on_token, stop_check,
                        logprobs, on_logprobs, on_done, stats_out))

    def stop(self):
        self.inbox.put(None)
        self.thread.join()

    def _admit(self, item):
        *request, on_done, stats_out = item
        try:
            seq = self.engine.submit(*request)
            if stats_out is not None:
                stats_out.append(seq.stats)
            self.active.append((seq, on_done))
        except Exception as e:  # noqa: BLE001  (e.g. prompt beyond seq_len)
            on_done(e)

    def _loop(self):
        while True:
            # block while there is nothing to step, else just drain
            try:
                item = self.inbox.get(block=self.engine.idle)
                if item is None:
                    return
                self._admit(item)
                continue
            except queue.Empty:
                pass
            try:
                self.engine.step()
                error = None
            except Exception as e:  # noqa: BLE001
                error = e
            still = []
            for seq, on_done in self.active:
                if error is not None or seq.done:
                    on_done(error)
                else:
                    still.append((seq, on_done))
            self.active = still
            if error is not None:
                # the engine's bookkeeping is no longer trustworthy
                m, tok = self.engine.model, self.engine.tokenizer
                self.engine = BatchEngine(m, tok, self.engine.n_batches)


class ApiState:
    def __init__(self, args):
        self.engine, self.m, self.comm = load_engine(args)
        # --slots > 1: requests decode together (load_engine has refused it
        # under tensor parallelism)
        self.scheduler = None
        if getattr(args, "slots", 1) > 1:
            self.scheduler = BatchScheduler(self.engine.model,
                                            self.engine.tokenizer,
                                            self.engine.n_batches)
        self.tok = self.engine.tokenizer
        eos_piece = (self.tok.vocab[self.tok.eos_token_ids[0]]
                     .decode("utf-8", "replace") if self.tok.eos_token_ids else "")
        self.template = ChatTemplateGenerator(TEMPLATE_UNKNOWN,
                                              self.tok.chat_template, eos_piece)
        self.cache = NaiveCache()
        self.model_name = "dllama"
        # per-request sampler defaults (reference re-parses params with CLI
        # defaults each request, dllama-api.cpp:491-520)
        self.default_temp = args.temperature
        self.default_topp = args.topp
        self.default_seed = args.seed if args.seed is not None else int(time.time())

    def complete(self, body: dict, emit, logprobs: int | None = None):
        """Run one chat completion; emit(delta_text) streams chunks. With
        logprobs = K (logprobs_requested) it is emit(delta_text, entries):
        the API's logprobs content of the tokens that delta released."""
        items = [ChatItem(m.get("role", "user"), m.get("content", ""))
                 for m in body.get("messages", [])]
        text = self.template.generate(items, True).content
        tokens = self.tok.encode(text)
        if self.scheduler is not None:
            return self._complete_batched(body, tokens, emit, logprobs)
        start = self.cache.resolve(tokens)
        self.engine.reset(start)
        max_tokens = int(body.get("max_tokens") or 256)
        # reset to CLI defaults so one request's overrides don't leak into the
        # next (reference dllama-api.cpp:491-520)
        self.engine.sampler.set_temp(self.default_temp)
        self.engine.sampler.topp = self.default_topp
        self.engine.sampler.set_seed(self.default_seed)
        if body.get("temperature") is not None:
            self.engine.sampler.set_temp(float(body["temperature"]))
        if body.get("top_p") is not None:
            self.engine.sampler.topp = float(body["top_p"])
        if body.get("seed") is not None:
            self.engine.sampler.set_seed(int(body["seed"]))
        user_stop = body.get("stop") or []
        if isinstance(user_stop, str):  # OpenAI allows string or list
            user_stop = [user_stop]
        stops = chat_stops(self.tok) + user_stop
        detector = EosDetector(self.tok.eos_token_ids, stops)
        self.tok.reset_decoder()
        deltas = _Deltas(self.tok, detector, emit, logprobs is not None)
        out_text = deltas.text
        more = ({} if logprobs is None else
                {"logprobs": logprobs, "on_logprobs": deltas.on_logprobs})
        gen_tokens, _ = self.engine.generate(
            tokens[start:], max_tokens, on_token=deltas.on_token,
            stop_check=lambda t: detector.is_eos(t) or detector.eos_pos >= 0,
            **more)
        deltas.finish()
        # cache only EVALUATED tokens: the last sampled token was never fed
        # through the model, so its KV row does not exist (reference caches
        # the evaluated endPos, dllama-api.cpp:470-473)
        self.cache.update(tokens + gen_tokens[:-1])
        return "".join(out_text), len(tokens), len(gen_tokens)


    def _complete_batched(self, body: dict, tokens: list, emit,
                          logprobs: int | None = None):
        """complete() in multi-slot mode: the request gets its own sampler,
        detector and streaming decoder, runs on the scheduler thread next to
        the other requests, and its deltas come back over a queue."""
        def param(name, default, cast):
            return cast(body[name]) if body.get(name) is not None else default

        sampler = Sampler(self.m.header.vocab_size,
                          param("temperature", self.default_temp, float),
                          param("top_p", self.default_topp, float),
                          param("seed", self.default_seed, int))
        user_stop = body.get("stop") or []
        if isinstance(user_stop, str):
            user_stop = [user_stop]
        detector = EosDetector(self.tok.eos_token_ids,
                               chat_stops(self.tok) + user_stop)
        tok = self.tok.fork_decoder()
        deltas: queue.Queue = queue.Queue()
        generated = [0]
        # runs on the scheduler thread: what it releases crosses the queue
        stream = _Deltas(tok, detector, lambda *released: deltas.put(released),
                         logprobs is not None)

        def on_token(t):
            generated[0] += 1
            stream.on_token(t)

        def on_done(error):
            if error is None:
                stream.finish()
            deltas.put(error if error is not None else StopIteration)

        stats = []
        self.scheduler.submit(
            tokens, int(body.get("max_tokens") or 256), sampler, on_token,
            lambda t: detector.is_eos(t) or detector.eos_pos >= 0,
            on_done, stats, logprobs,
            stream.on_logprobs if logprobs is not None else None)
        out_text = []
        while True:
            item = deltas.get()
            if item is StopIteration:
                break
            if isinstance(item, Exception):
                raise item
            out_text.append(item[0])
            emit(*item)
        # a fourth value on this path only: the prompt tokens that came from
        # shared KV pages (0 on an unpaged model)
        return ("".join(out_text), len(tokens), generated[0],
                stats[0].cached_tokens if stats else 0)


STATE: ApiState | None = None


class Handler(BaseHTTPRequestHandler):
    protocol_version = "HTTP/1.1"

    def log_message(self, fmt, *a):  # quiet
        pass

    def _json(self, code: int, obj: dict):
        data = json.dumps(obj).encode()
        self.send_response(code)
        self.send_header("Content-Type", "application/json")
        self.send_header("Content-Length", str(len(data)))
        self.end_headers()
        self.wfile.write(data)

    def do_GET(self):
        if self.path == "/v1/models":
            self._json(200, {"object": "list", "data": [
                {"id": STATE.model_name, "object": "model",
                 "created": int(time.time()), "owned_by": "dllama_amd"}]})
        elif self.path == "/health":
            self._json(200, {"status": "ok"})
        else:
            self._json(404, {"error": "not found"})

    def do_POST(self):
        if self.path not in ("/v1/chat/completions", "/chat/completions"):
            self._json(404, {"error": "not found"})
            return
        length = int(self.headers.get("Content-Length", 0))
        try:
            body = json.loads(self.rfile.read(length) or b"{}")
        except json.JSONDecodeError:
            self._json(400, {"error": "invalid json"})
            return
        try:
            logprobs = logprobs_requested(body, STATE.comm.world)
        except BadRequest as e:
            self._json(400, {"error": {
                "message": str(e), "type": "invalid_request_error",
                "param": e.param, "code": None}})
            return
        rid = f"chatcmpl-{uuid.uuid4().hex[:12]}"
        created = int(time.time())
        stream = bool(body.get("stream"))
        if stream:
            self.send_response(200)
            self.send_header("Content-Type", "text/event-stream")
            self.send_header("Cache-Control", "no-cache")
            self.send_header("Transfer-Encoding", "chunked")
            self.end_headers()

            def emit(delta, entries=None):
                choice = {"index": 0, "delta": {"content": delta},
                          "finish_reason": None}
                if entries is not None:
                    choice["logprobs"] = {"content": entries}
                chunk = {"id": rid, "object": "chat.completion.chunk",
                         "created": created, "model": STATE.model_name,
                         "choices": [choice]}
                self._chunk(f"data: {json.dumps(chunk)}\n\n")

            try:
                STATE.complete(body, emit, logprobs)
            finally:
                fin = {"id": rid, "object": "chat.completion.chunk",
                       "created": created, "model": STATE.model_name,
                       "choices": [{"index": 0, "delta": {},
                                    "finish_reason": "stop"}]}
                self._chunk(f"data: {json.dumps(fin)}\n\n")
                self._chunk("data: [DONE]\n\n")
                self.wfile.write(b"0\r\n\r\n")
        else:
            content = []
            try:
                text, n_prompt, n_gen, *cached = STATE.complete(
                    body, lambda d, entries=(): content.extend(entries),
                    logprobs)
            except Exception as e:  # noqa: BLE001
                self._json(500, {"error": {"message": str(e), "type": "server_error"}})
                return
            usage = {"prompt_tokens": n_prompt, "completion_tokens": n_gen,
                     "total_tokens": n_prompt + n_gen}
            if cached:  # the batched path
                usage["prompt_tokens_details"] = {"cached_tokens": cached[0]}
            choice = {"index": 0, "message":
                      {"role": "assistant", "content": text},
                      "finish_reason": "stop"}
            if logprobs is not None:
                choice["logprobs"] = {"content": content}
            self._json(200, {
                "id": rid, "object": "chat.completion", "created": created,
                "model": STATE.model_name,
                "choices": [choice],
                "usage": usage})

    def _chunk(self, s: str):
        data = s.encode()
        self.wfile.write(f"{len(data):x}\r\n".encode() + data + b"\r\n")
        self.wfile.flush()


def main(argv=None) -> int:
    global STATE
    parser = build_parser()
    args = parser.parse_args(["inference"] + (argv if argv is not None
                                              else sys.argv[1:]))
    STATE = ApiState(args)
    comm = STATE.comm
    if comm.world > 1:
        # TP serving: rank 0 owns HTTP + sampling; ranks > 0 replay control
        # packets (reference root/worker split, app.cpp:168-230) — without
        # this every rank would bind the port
        from ..parallel.lockstep import RootModel, follower_loop
        if comm.rank > 0:
            follower_loop(STATE.engine.model, comm)
            return 0
        STATE.engine.model = RootModel(STATE.engine.model, comm)
    multi = STATE.scheduler is not None
    server = (ThreadingHTTPServer if multi else HTTPServer)(
        (args.host, args.port), Handler)
    print(f"⭐ dllama-api listening on {args.host}:{args.port}")
    try:
        server.serve_forever()
    except KeyboardInterrupt:
        pass
    finally:
        if comm.world > 1 and comm.rank == 0:
            STATE.engine.model.stop_followers()
        if multi:
            STATE.scheduler.stop()
    return 0


if __name__ == "__main__":
    sys.exit(main())
