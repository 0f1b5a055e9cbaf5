"""Continuous batching: a static slot pool and a one-thread scheduler.

A pool holds ``max_batch`` sequences in one preallocated
[max_batch, Hkv, capacity, D] cache per layer.  Every slot has its own
position, kept on device (int32 [max_batch]).  A request is prefilled
alone into a free slot through a B=1 view of the pool (``KVCache.slot``),
then every decode step advances ALL slots in one batched forward: the
decode kernels read row b's position from ``pos[b]``.  B and every
buffer are fixed, so the step is captured in one hipGraph and replayed.

Idle slots feed token 0 with their position pinned at 0: they rewrite
row 0 of their own slot and attend over one key.  Their work is real
(MoE expert traffic included) — the price of a fixed-shape graph.
"""

from __future__ import annotations

import os
import queue
import sys
import threading
from collections import deque
from typing import Deque, List, Optional, Tuple

import torch

from .. import ops
from ..utils import metrics
from .engine import SamplingParams

MAX_BATCH_LIMIT = 64     # the M<=64 decode-GEMM regime
GRAPH_MAX_BATCH = 16     # capture the step only up to this batch

_END = object()


def env_max_batch() -> int:
    """Default of the servers' ``--max-batch`` (MLXS_MAX_BATCH, else 1)."""
    return int(os.environ.get("MLXS_MAX_BATCH", "1"))


def max_batch_of(args) -> int:
    """Validated ``max_batch`` of a CLI namespace; 1 (no batching) when
    the namespace predates the flag."""
    n = int(getattr(args, "max_batch", 1) or 1)
    if not 1 <= n <= MAX_BATCH_LIMIT:
        raise ValueError(f"--max-batch must be in [1, {MAX_BATCH_LIMIT}], "
                         f"got {n}")
    return n


def serve_capacity() -> int:
    """Positions per slot (MLXS_AMD_SERVE_CAPACITY, as for the B=1
    serving graph)."""
    return int(os.environ.get("MLXS_AMD_SERVE_CAPACITY", "4096"))


def plain_greedy(params: SamplingParams) -> bool:
    """Argmax of the unedited logits: such rows share one batched
    on-device argmax."""
    return (params.temperature <= 0.0 and not params.logit_bias
            and not (params.repetition_penalty
                     and params.repetition_penalty != 1.0))


def penalty_window(params: SamplingParams) -> Optional[int]:
    """Tokens of context the request's repetition penalty looks at: 0
    without a penalty, None when the whole context counts."""
    if not (params.repetition_penalty
            and params.repetition_penalty != 1.0):
        return 0
    return params.repetition_context_size or None


def device_sampled(params: SamplingParams, *, on_gpu: bool, native: bool,
                   disabled: bool) -> bool:
    """Whether a request's rows are sampled by the batched
    ``ops.sample_rows`` kernel.  on_gpu: the pool is on a GPU; native: the
    HIP extension is live (not MLXS_AMD_FORCE_TORCH); disabled:
    MLXS_AMD_NO_FUSED_SAMPLE is set.  Seeded requests draw from their CPU
    generator and plain-greedy ones from the batched argmax; a bias table
    or penalty window beyond the kernel's limits keeps the per-row path."""
    window = penalty_window(params)
    return (on_gpu and native and not disabled
            and params.seed is None
            and not plain_greedy(params)
            and len(params.logit_bias or ()) <= ops.SAMPLE_ROWS_MAX_BIAS
            and window is not None
            and window <= ops.SAMPLE_ROWS_MAX_WINDOW)


def fused_sample_disabled() -> bool:
    return bool(os.environ.get("MLXS_AMD_NO_FUSED_SAMPLE"))


class _Request:
    def __init__(self, prompt_ids: List[int], params: SamplingParams):
        self.prompt = prompt_ids
        self.params = params
        self.q: "queue.Queue" = queue.Queue()
        self.closed = False
        self.n_out = 0
        self.rep_context: List[int] = list(prompt_ids)
        self.gen = None
        if params.seed is not None:
            self.gen = torch.Generator(device="cpu").manual_seed(params.seed)
        # plain greedy rows share one batched on-device argmax
        self.plain_greedy = plain_greedy(params)
        # sampled by ops.sample_rows; decided at admission
        self.on_device = False


class _RowSampler:
    """Device state of the batched sampler: per-slot parameter vectors
    (written at admission, cleared at release), the uniform draws and the
    logsumexp the kernel leaves for the streams' logprobs."""

    def __init__(self, B: int, dev):
        NB, W = ops.SAMPLE_ROWS_MAX_BIAS, ops.SAMPLE_ROWS_MAX_WINDOW
        f32, i32 = torch.float32, torch.int32
        self.temperature = torch.zeros(B, dtype=f32, device=dev)
        self.top_p = torch.ones(B, dtype=f32, device=dev)
        self.penalty = torch.ones(B, dtype=f32, device=dev)
        self.active = torch.zeros(B, dtype=i32, device=dev)
        self.u = torch.zeros(B, dtype=f32, device=dev)
        self.lse = torch.zeros(B, dtype=f32, device=dev)
        self.bias_idx = torch.full((B, NB), -1, dtype=i32, device=dev)
        self.bias_val = torch.zeros(B, NB, dtype=f32, device=dev)
        self.pen_idx = torch.full((B, W), -1, dtype=i32, device=dev)
        self.one = torch.ones(1, dtype=i32, device=dev)
        self.rows: set = set()        # slots of device-sampled requests
        self.bias_rows: set = set()   # ... with a logit_bias
        self.pen_rows: set = set()    # ... with a repetition penalty

    def admit(self, b: int, p: SamplingParams):
        self.rows.add(b)
        self.temperature[b].fill_(max(float(p.temperature), 0.0))
        self.top_p[b].fill_(float(p.top_p))
        self.active[b].fill_(1)
        if p.logit_bias:
            n = len(p.logit_bias)
            self.bias_idx[b, :n].copy_(torch.tensor(
                list(p.logit_bias.keys()), dtype=torch.int32), True)
            self.bias_val[b, :n].copy_(torch.tensor(
                list(p.logit_bias.values()), dtype=torch.float32), True)
            self.bias_rows.add(b)
        if penalty_window(p):
            self.penalty[b].fill_(float(p.repetition_penalty))
            self.pen_rows.add(b)

    def release(self, b: int):
        if b not in self.rows:
            return
        self.rows.discard(b)
        self.temperature[b].zero_()
        self.top_p[b].fill_(1.0)
        self.active[b].zero_()
        if b in self.bias_rows:
            self.bias_rows.discard(b)
            self.bias_idx[b].fill_(-1)
            self.bias_val[b].zero_()
        if b in self.pen_rows:
            self.pen_rows.discard(b)
            self.penalty[b].fill_(1.0)
            self.pen_idx[b].fill_(-1)

    @staticmethod
    def _window(req: "_Request") -> List[int]:
        W = ops.SAMPLE_ROWS_MAX_WINDOW
        win = req.rep_context[-req.params.repetition_context_size:]
        return win + [-1] * (W - len(win))

    def sample(self, logits: torch.Tensor, tok: torch.Tensor, slots,
               b: Optional[int] = None):
        """One launch over the pool's logits [B, V] (b is None), or over
        the [1, V] prefill logits of slot ``b``.  Leaves the ids in
        ``tok`` and the logsumexp of the edited rows in ``self.lse``."""
        W = ops.SAMPLE_ROWS_MAX_WINDOW
        rows = slice(None) if b is None else slice(b, b + 1)
        pen_rows = self.pen_rows if b is None else self.pen_rows & {b}
        bias_rows = self.bias_rows if b is None else self.bias_rows & {b}
        self.u[rows].uniform_()
        if pen_rows:
            # the windows move every step: one upload for the batch
            pad = [-1] * W
            host = [self._window(slots[i]) if i in pen_rows else pad
                    for i in (range(len(slots)) if b is None else (b,))]
            self.pen_idx[rows].copy_(
                torch.tensor(host, dtype=torch.int32), non_blocking=True)
        ops.sample_rows(
            logits, self.temperature[rows], self.top_p[rows], self.u[rows],
            self.active if b is None else self.one, tok[rows],
            self.lse[rows],
            self.bias_idx[rows] if bias_rows else None,
            self.bias_val[rows] if bias_rows else None,
            self.pen_idx[rows] if pen_rows else None,
            self.penalty[rows] if pen_rows else None)


class TokenStream:
    """Iterator of (token_id, logprobs[V]) with generator semantics:
    ``close()`` (or dropping the last reference) releases the slot at
    the scheduler's next step boundary."""

    def __init__(self, sched: "BatchScheduler", req: _Request):
        self._sched = sched
        self._req = req
        self._done = False

    def __iter__(self):
        return self

    def __next__(self) -> Tuple[int, torch.Tensor]:
        if self._done:
            raise StopIteration
        item = self._req.q.get()
        if item is _END:
            self._done = True
            raise StopIteration
        if isinstance(item, BaseException):
            self._done = True
            raise item
        return item

    def close(self):
        self._done = True
        if not self._req.closed:
            self._req.closed = True
            self._sched._wake()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter teardown
            pass


class BatchScheduler:
    """Slot scheduler for a single-stage model (see module docstring).

    ``submit`` may be called from any thread; one scheduler thread owns
    all model and device work."""

    def __init__(self, model, max_batch: int, capacity: int, device=None,
                 prefill_chunk: int = 0):
        if not 1 <= max_batch <= MAX_BATCH_LIMIT:
            raise ValueError(f"max_batch must be in [1, {MAX_BATCH_LIMIT}], "
                             f"got {max_batch}")
        if capacity < 2:
            raise ValueError("capacity must be at least 2")
        shard = getattr(model, "shard", None)
        if shard is not None and not (shard.is_first and shard.is_last):
            raise ValueError("BatchScheduler needs a single-stage model")
        self.model = model
        self.max_batch = max_batch
        self.capacity = capacity
        self.device = torch.device(
            device if device is not None
            else next(model.parameters()).device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.prefill_chunk = prefill_chunk
        B, dev = max_batch, self.device
        self.caches = model.make_cache(batch_size=B, device=dev)
        for c in self.caches:
            c.allocate(capacity, B)
        # device-resident step state: input token, position and the 0/1
        # position increment of every slot
        self.tok = torch.zeros(B, 1, dtype=torch.int64, device=dev)
        self.pos = torch.zeros(B, dtype=torch.int32, device=dev)
        self.inc = torch.zeros(B, dtype=torch.int32, device=dev)
        for c in self.caches:
            c.graph_pos = self.pos
        self._slots: List[Optional[_Request]] = [None] * B
        self._pos_host = [0] * B
        self._pending: Deque[_Request] = deque()
        self._cv = threading.Condition()
        self._stop = False
        self._error: Optional[BaseException] = None
        self._graph = None
        self._logits_out: Optional[torch.Tensor] = None
        self.graphed = False
        # batched sampler state; only where ops.sample_rows has a kernel
        self._sampler: Optional[_RowSampler] = (
            _RowSampler(B, dev) if ops.use_native(self.tok) else None)
        self._m = metrics.batching_metrics()
        self._thread = threading.Thread(target=self._run, daemon=True,
                                        name="batch-scheduler")
        self._thread.start()

    # -- public ------------------------------------------------------------
    def submit(self, prompt_ids, params: Optional[SamplingParams] = None
               ) -> TokenStream:
        """Queue a request; returns its (token_id, logprobs[V]) stream —
        the ``engine.generate_step`` contract.  The stream ends on its
        own at ``params.max_tokens`` (when set) or when the slot is full."""
        ids = [int(t) for t in (prompt_ids.reshape(-1).tolist()
                                if torch.is_tensor(prompt_ids)
                                else prompt_ids)]
        self.check_prompt(len(ids))
        req = _Request(ids, params or SamplingParams())
        with self._cv:
            if self._error is not None:
                req.q.put(self._failure())
            elif self._stop:
                req.q.put(RuntimeError("batch scheduler is shut down"))
            else:
                self._pending.append(req)
                self._m["queued"].set(len(self._pending))
                self._cv.notify_all()
        return TokenStream(self, req)

    def check_prompt(self, n_tokens: int):
        if n_tokens < 1:
            raise ValueError("prompt must hold at least one token")
        if n_tokens > self.capacity - 1:
            raise ValueError(
                f"prompt of {n_tokens} tokens exceeds the slot capacity "
                f"({self.capacity - 1} prompt tokens at most)")

    def close(self):
        with self._cv:
            self._stop = True
            self._cv.notify_all()
        self._thread.join(timeout=30)

    # -- scheduler thread ----------------------------------------------------
    def _wake(self):
        with self._cv:
            self._cv.notify_all()

    def _failure(self) -> BaseException:
        e = RuntimeError(f"batch scheduler failed: {self._error!r}")
        e.__cause__ = self._error
        return e

    def _run(self):
        try:
            if self.device.type == "cuda":
                torch.cuda.set_device(self.device)
            with torch.no_grad():
                self._maybe_capture()
                while True:
                    with self._cv:
                        while (not self._stop and not self._pending
                               and not any(self._slots)):
                            self._cv.wait()
                        if self._stop:
                            break
                    self._iteration()
            err: Optional[BaseException] = None
        except BaseException as e:  # noqa: BLE001 — delivered to the waiters
            err = e
        with self._cv:
            self._error = err
            self._stop = True
            waiters = [r for r in self._slots if r is not None]
            waiters += list(self._pending)
            self._pending.clear()
            self._slots = [None] * self.max_batch
            for r in waiters:
                r.q.put(self._failure() if err is not None else _END)
            self._m["active_slots"].set(0)
            self._m["queued"].set(0)

    def _iteration(self):
        # step boundary: free the slots whose stream was closed
        for b, r in enumerate(self._slots):
            if r is not None and r.closed:
                self._release(b)
        # admit at most one request, so running streams stall for one
        # prefill at the most
        req = None
        with self._cv:
            while self._pending and None in self._slots:
                cand = self._pending.popleft()
                if not cand.closed:
                    req = cand
                    break
            self._m["queued"].set(len(self._pending))
        if req is not None:
            self._admit(self._slots.index(None), req)
        self._m["active_slots"].set(sum(r is not None for r in self._slots))
        if any(self._slots):
            self._decode()
            self._m["active_slots"].set(
                sum(r is not None for r in self._slots))

    def _release(self, b: int):
        self._slots[b] = None
        self._pos_host[b] = 0
        if self._sampler is not None:
            self._sampler.release(b)
        self.tok[b].zero_()
        self.pos[b].zero_()
        self.inc[b].zero_()

    def _admit(self, b: int, req: _Request):
        """Prefill ``req`` alone through the B=1 view of slot ``b``."""
        self._slots[b] = req  # owned from here on: a failure reaches it
        view = [c.slot(b) for c in self.caches]
        ids = torch.tensor([req.prompt], dtype=torch.long, device=self.device)
        T = ids.shape[1]
        chunk = self.prefill_chunk
        if chunk and T > chunk:
            for c0 in range(0, T, chunk):
                h = self.model(ids[:, c0: c0 + chunk], view)
        else:
            h = self.model(ids, view)
        self._pos_host[b] = T
        self.pos[b].fill_(T)
        self.inc[b].fill_(1)
        logits = h[:, -1, :].float()
        req.on_device = self._on_device(req.params, logits.shape[-1])
        if req.on_device:
            # the first token through the batched sampler at B = 1
            self._sampler.admit(b, req.params)
            logits = logits.contiguous()
            self._sampler.sample(logits, self.tok, self._slots, b)
            self._emit(b, req, logits, None, int(self.tok[b].item()), row=0,
                       fed=True)
            return
        lse = torch.logsumexp(logits, dim=-1, keepdim=True)
        am = logits.argmax(-1).tolist() if req.plain_greedy else None
        self._emit(b, req, logits, lse, am[0] if am else None, row=0,
                   fed=False)

    def _on_device(self, p: SamplingParams, vocab: int) -> bool:
        return (self._sampler is not None
                and device_sampled(p, on_gpu=True,
                                   native=ops.use_native(self.tok),
                                   disabled=fused_sample_disabled())
                # the per-row path wraps negative keys and raises on
                # keys past the vocabulary: leave both to it
                and all(0 <= int(k) < vocab for k in (p.logit_bias or ())))

    def _step(self) -> torch.Tensor:
        h = self.model(self.tok, self.caches)
        logits = h[:, -1, :].float()
        self.pos.add_(self.inc)
        return logits

    def _decode(self):
        if self._graph is not None:
            self._graph.replay()
            logits = self._logits_out
        else:
            logits = self._step()
        self._m["decode_steps"].inc()
        lse = torch.logsumexp(logits, dim=-1, keepdim=True)
        am = logits.argmax(-1)
        # greedy feed for every running row in one device op (inc masks
        # idle rows back to token 0); other rows are overwritten below
        self.tok.copy_((am * self.inc).view(-1, 1))
        if self._sampler is not None and self._sampler.rows:
            # one launch samples every device row into tok, over the
            # greedy feed; greedy rows read their argmax back from tok too
            # (inc is 1 on every running row), so the step still has one
            # readback
            self._sampler.sample(logits, self.tok, self._slots)
            am_host = self.tok.view(-1).tolist()
        else:
            am_host = am.tolist()
        for b, req in enumerate(self._slots):
            if req is None:
                continue
            self._pos_host[b] += 1
            self._emit(b, req, logits, lse, am_host[b], row=b,
                       fed=req.plain_greedy or req.on_device)

    def _emit(self, b: int, req: _Request, logits: torch.Tensor,
              lse: torch.Tensor, greedy_tok: Optional[int], row: int,
              fed: bool):
        """Sample slot ``b``'s next token from ``logits[row]``, hand it to
        the request and make it the slot's next input (``fed``: the
        batched argmax or the batched sampler already wrote it;
        ``greedy_tok`` is that token)"""
        p = req.params
        if req.plain_greedy:
            tid = greedy_tok
            logprobs = logits[row] - lse[row]
        elif req.on_device:
            # sample_rows edited the row in place and left its logsumexp
            tid = greedy_tok
            logprobs = logits[row] - self._sampler.lse[b]
        else:
            # the per-request path of engine.generate_step
            lg = logits[row: row + 1].clone()
            if p.logit_bias:
                idx = torch.tensor(list(p.logit_bias.keys()),
                                   device=lg.device)
                vals = torch.tensor(list(p.logit_bias.values()),
                                    device=lg.device, dtype=lg.dtype)
                lg[0, idx] += vals
            if p.repetition_penalty and p.repetition_penalty != 1.0:
                window = req.rep_context[-p.repetition_context_size:] \
                    if p.repetition_context_size else req.rep_context
                ctx = torch.tensor(window, device=lg.device, dtype=torch.long)
                lg = ops.apply_repetition_penalty(lg, ctx,
                                                  p.repetition_penalty)
            logprobs = (lg - torch.logsumexp(lg, dim=-1, keepdim=True))[0]
            if req.gen is not None and lg.is_cuda:
                # seeded sampling draws from the CPU generator, so a
                # seed reproduces across devices
                tid = int(ops.sample(lg.cpu(), p.temperature, p.top_p,
                                     req.gen).item())
            else:
                tid = int(ops.sample(lg, p.temperature, p.top_p,
                                     req.gen).item())
        if not fed:
            self.tok[b].fill_(tid)
        req.rep_context.append(tid)
        req.n_out += 1
        req.q.put((tid, logprobs))
        # hard stops: the request's own token budget, and a full slot —
        # at pos == capacity-1 the next append would be the last row; the
        # stream ends here and the slot never issues another append
        if ((p.max_tokens is not None and req.n_out >= p.max_tokens)
                or self._pos_host[b] >= self.capacity - 1):
            req.q.put(_END)
            self._release(b)

    # -- hipGraph ------------------------------------------------------------
    def _maybe_capture(self):
        """Capture the batched step once (side-stream warm-up, static
        input/output buffers).  Runs before any admission, so every slot
        is idle: the warm-up and capture steps only rewrite row 0."""
        if (self.device.type != "cuda" or self.max_batch > GRAPH_MAX_BATCH
                or os.environ.get("MLXS_AMD_SERVE_GRAPH", "1") == "0"):
            return
        try:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):
                    self._step()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = self._step()
            self._graph, self._logits_out = g, out
            self.graphed = True
        except Exception as e:  # noqa: BLE001
            print(f"batched decode graph capture failed, eager decode: {e}",
                  file=sys.stderr, flush=True)
            self._graph = None
            self._logits_out = None
