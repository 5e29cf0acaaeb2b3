"""Device-resident state of temperature / top-p sampling in the decode loops (K11 of include/magicdec_hip.h).

The reference defines the sampling semantics (Engine/utils.py:68-98: get_sampling_logits / sample) but decodes greedily
in every speculative loop.  A Sampler attached to a model (attach()) replaces the model's argmax by a draw, according
to the role its back-end set for the step:

* "prefill"  (last prefill chunk) and "baseline" (autoregressive step): one draw per request;
* "draft"    (a draft step): one draw per request, and the row plus its stats go to slot j of the draft ring;
* "verify"   (the gamma+1-row target step): the speculative-sampling verify kernel, whose output is the target_tokens
  tensor the unchanged accept kernel consumes.

Everything the kernels read lives here, allocated once, before any graph capture: the iteration counter and the
draft-step index are device tensors the kernels advance themselves, so one captured graph per step serves every
iteration.  Sampler holds one temperature / top_p per run (changing them after a capture needs clear_graphs());
RequestSampler holds a temperature, a top_p and a top_k per request in device tensors the kernels read at launch time,
so they change under captured graphs, and a batch may mix greedy and sampled requests.

Sampler and RequestSampler are the one-GPU forms and reject tensor-parallel models.  ShardedSampler is the opt-in form
for a vocab-sharded lm head (Engine/tp.py:apply_tp): the same semantics and the same bits, as a chain of local launches
with one small all-reduce between two of them (K11 "sharded": 4 collectives per call, 3 at top_p = 1).  The phases are
validated with the ranks emulated in one process on one GPU, the class by two processes sharing one GPU over gloo
(tests/test_gpu_sampling_tp.py); nothing here has run across physical GPUs.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from .. import ops, sampling_ops

ROLES = ("prefill", "baseline", "draft", "verify")


def validate(temperature, top_p):
    if not temperature >= 0:
        raise ValueError(f"temperature must be >= 0, got {temperature}")
    if not 0 < top_p <= 1:
        raise ValueError(f"top_p must be in (0, 1], got {top_p}")


class Sampler:
    def __init__(self, temperature, top_p, seed, B, gamma, vocab, device):
        validate(temperature, top_p)
        if temperature == 0:
            raise ValueError("temperature 0 is greedy decoding: run without a Sampler")
        self.temperature, self.top_p = float(temperature), float(top_p)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.B, self.gamma, self.vocab = B, gamma, vocab
        dev = torch.device(device)
        self.counters = torch.zeros(4, dtype=torch.int32, device=dev)        # iteration, draft step, ticket, -
        self.row_sel = torch.ones(B, dtype=torch.int64, device=dev)          # two-token draft step: row cachelens_update-1
        g = max(gamma, 1)
        self.ring = torch.zeros((B, g, vocab), dtype=torch.bfloat16, device=dev)
        self.ring_stats = torch.zeros((B, g, ops.STATS_WORDS), dtype=torch.int64, device=dev)
        self.target_stats = torch.zeros((B * (g + 1), ops.STATS_WORDS), dtype=torch.int64, device=dev)
        self.captured = False           # set by Engine/graph.py when a step with this sampler was captured

    def set_params(self, temperature, top_p):
        assert not self.captured, "temperature / top_p are baked into the captured steps: call clear_graphs() first"
        validate(temperature, top_p)
        if temperature == 0:
            raise ValueError("temperature 0 is greedy decoding: detach the Sampler instead")
        self.temperature, self.top_p = float(temperature), float(top_p)

    def reset(self, seed=None):
        """Restart the noise stream (iteration 0, draft step 0), optionally with another seed (graph-safe: in place)."""
        if seed is not None:
            assert not self.captured, "the seed is baked into the captured steps: call clear_graphs() first"
            self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.counters.zero_()

    # graph capture runs a step twice as a warm-up: those runs must not advance the stream
    def save(self):
        return self.counters.clone()

    def restore(self, saved):
        self.counters.copy_(saved)

    def check_model(self, model):
        if getattr(model, "process_group", None) is not None:
            raise ValueError("sampling supports TP = 1 only (the vocab-sharded version needs cross-rank max / Z / "
                             "histogram reductions)")
        vocab = model.output.weight.shape[0]
        if vocab != self.vocab:
            raise ValueError(f"sampling: the model's vocabulary ({vocab}) differs from the sampler's ({self.vocab}); "
                             "draft and target vocabulary sizes must be equal")

    def head(self, logits, role, idx, B, n):
        """The draw that replaces Transformer._argmax for one step: [B, n] int64 tokens."""
        T, p, s = self.temperature, self.top_p, self.seed
        if role == "verify":
            if n != self.gamma + 1:
                raise ValueError(f"verify step with {n} rows per request, sampler gamma = {self.gamma}")
            return ops.spec_verify_sample(logits, idx, self.ring, self.ring_stats, self.target_stats, self.counters,
                                          T, p, s)
        if role == "draft":
            return ops.sample_rows(logits, n, T, p, s, ops.SAMPLE_DRAFT, self.counters, ops.ADVANCE_STEP,
                                   row_sel=self.row_sel if n == 2 else None, ring=self.ring,
                                   ring_stats=self.ring_stats)
        if role in ("prefill", "baseline"):
            purpose = ops.SAMPLE_PREFILL if role == "prefill" else ops.SAMPLE_BASELINE
            return ops.sample_rows(logits, n, T, p, s, purpose, self.counters, ops.ADVANCE_ITER)
        raise ValueError(f"sampling: step role {role!r} is not one of {ROLES}")


def _per_request(name, value, B, low_ok, what):
    """A scalar or a length-B sequence -> list of B host values, each passing `low_ok`."""
    vals = [value] * B if not hasattr(value, "__len__") else list(value)
    if len(vals) != B:
        raise ValueError(f"{name}: {len(vals)} values for {B} requests")
    for v in vals:
        if not low_ok(v):
            raise ValueError(f"{name} must be {what}, got {v}")
    return vals


def _temperature_ok(v):
    """0 (greedy), or a value whose fp32 form is finite and positive with a finite fp32 reciprocal: the kernels compute
    invT = fp32(1 / T), and an infinite or zero invT turns the masses into NaN or all-equal."""
    if not v >= 0:
        return False
    if v == 0:
        return True
    t = torch.tensor(float(v), dtype=torch.float32)
    return bool(torch.isfinite(t) and t > 0 and torch.isfinite(1.0 / t))


class RequestSampler(Sampler):
    """Sampler whose temperature, top_p and top_k are per request (K11 "per request"): three [B] device tensors,
    allocated once and read by the kernels at launch time.  set_params() copies new values in place and is allowed after
    a capture -- the captured steps hold the tensors, not the values.  temperature 0 makes a request greedy (its tokens
    are the argmax of its rows, its verify row what the greedy loop hands the accept kernel), so a batch may mix greedy
    and sampled requests, and an all-greedy batch is legal; top_k 0 is off.  One seed per run.

    One rank only.  The sharded phases (ShardedSampler) keep one (temperature, top_p) per run and have no top-k: that
    needs a count histogram through phases B / C and their collectives, which is not built."""

    def __init__(self, temperature, top_p, top_k, seed, B, gamma, vocab, device):
        Sampler.__init__(self, 1.0, 1.0, seed, B, gamma, vocab, device)
        dev = torch.device(device)
        self.T = torch.zeros(B, dtype=torch.float32, device=dev)
        self.P = torch.ones(B, dtype=torch.float32, device=dev)
        self.K = torch.zeros(B, dtype=torch.int32, device=dev)
        self.set_params(temperature, top_p, top_k)

    def set_params(self, temperature, top_p, top_k=0):
        """Each a scalar or a length-B sequence; validated on the host, copied in place (graph-safe)."""
        B = self.B
        t = _per_request("temperature", temperature, B, _temperature_ok,
                         ">= 0 and, unless 0, finite in fp32 with a finite fp32 reciprocal")
        p = _per_request("top_p", top_p, B, lambda v: 0 < v <= 1, "in (0, 1]")
        k = _per_request("top_k", top_k, B, lambda v: int(v) == v and v >= 0, "an integer >= 0 (0 = off)")
        self.temperature, self.top_p, self.top_k = [float(v) for v in t], [float(v) for v in p], [int(v) for v in k]
        self.T.copy_(torch.tensor(self.temperature, dtype=torch.float32))
        self.P.copy_(torch.tensor(self.top_p, dtype=torch.float32))
        self.K.copy_(torch.tensor([min(v, 0x7FFFFFFF) for v in self.top_k], dtype=torch.int32))

    def check_model(self, model):
        if getattr(model, "process_group", None) is not None:
            raise ValueError("per-request sampling supports TP = 1 only: the vocab-sharded phases take one "
                             "(temperature, top_p) per run and have no top-k (no count histogram through their "
                             "collectives)")
        Sampler.check_model(self, model)

    def head(self, logits, role, idx, B, n):
        if B != self.B:
            raise ValueError(f"per-request sampling: step of {B} requests, the sampler was built for {self.B}")
        T, p, k, s = self.T, self.P, self.K, self.seed
        if role == "verify":
            if n != self.gamma + 1:
                raise ValueError(f"verify step with {n} rows per request, sampler gamma = {self.gamma}")
            return sampling_ops.spec_verify_sample_req(logits, idx, self.ring, self.ring_stats, self.target_stats,
                                                       self.counters, T, p, k, s)
        if role == "draft":
            return sampling_ops.sample_rows_req(logits, n, T, p, k, s, ops.SAMPLE_DRAFT, self.counters,
                                                ops.ADVANCE_STEP, row_sel=self.row_sel if n == 2 else None,
                                                ring=self.ring, ring_stats=self.ring_stats)
        if role in ("prefill", "baseline"):
            purpose = ops.SAMPLE_PREFILL if role == "prefill" else ops.SAMPLE_BASELINE
            return sampling_ops.sample_rows_req(logits, n, T, p, k, s, purpose, self.counters, ops.ADVANCE_ITER)
        raise ValueError(f"sampling: step role {role!r} is not one of {ROLES}")


def shard_offsets(widths):
    """Exclusive prefix sum of the ranks' local vocabulary widths -> (offsets, total).  The widths need not be equal:
    torch.chunk (Engine/tp.py) gives the last rank fewer columns."""
    offs, tot = [], 0
    for w in widths:
        if w < 1:
            raise ValueError(f"sharded sampling: a rank holds no vocabulary columns (widths {list(widths)})")
        offs.append(tot)
        tot += int(w)
    return offs, tot


def _group_ranks(group):
    """The global ranks of `group`, or None when this rank is outside it (torch raises ValueError / KeyError)."""
    try:
        return tuple(dist.get_process_group_ranks(group))
    except (ValueError, KeyError, RuntimeError, TypeError, AttributeError):
        return None


def _same_ranks(a, b):
    ra, rb = _group_ranks(a), _group_ranks(b)
    return ra is not None and ra == rb          # a group this rank cannot see matches nothing


class ShardedSampler(Sampler):
    """Sampler for a model whose lm head is vocab-sharded over `group`: rank r holds the logits columns
    [vocab_offset, vocab_offset + v_loc).  head() runs launch -> all_reduce(MAX | SUM) -> launch ... on device tensors
    allocated here; nothing is read back to the host (the returned token tensor is the only per-step allocation, as in
    the base class).

    The draft of a longspec run is either sharded over the same ranks as the target (ring shard [B, gamma, v_loc]) or,
    with replicate_draft, whole on every rank (full ring [B, gamma, vocab], drawn by the one-GPU md_sample_rows, which
    is bit-identical on every rank).  A draft sharded over a sub-group of the target's ranks is NOT supported: the ranks
    outside the sub-group have no ring to verify against (it would have to be all-gathered to them).

    The sharded phases stay scalar-parameter: one (temperature, top_p) per run and no top-k.  Per-request values and a
    top-k select (RequestSampler) would need a count histogram through phases B / C and their collectives; not built."""

    def __init__(self, temperature, top_p, seed, B, gamma, v_loc, device, group, replicate_draft=False):
        self.group = group
        dev = torch.device(device)
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        mine = torch.tensor([v_loc], dtype=torch.int64, device=dev)
        parts = [torch.zeros_like(mine) for _ in range(self.world)]
        dist.all_gather(parts, mine, group=group)
        widths = [int(t.item()) for t in parts]
        offs, total = shard_offsets(widths)
        if widths[self.rank] != v_loc:
            raise ValueError(f"sharded sampling: rank {self.rank} holds {v_loc} columns, the group says {widths[self.rank]}")
        self.v_loc, self.vocab_offset, self.vocab_total = int(v_loc), offs[self.rank], total
        self.replicate_draft = bool(replicate_draft)
        super().__init__(temperature, top_p, seed, B, gamma, total if replicate_draft else v_loc, device)
        self.vocab = total
        g = max(gamma, 1)
        i64 = dict(dtype=torch.int64, device=dev)
        R = B * (g + 1)
        # reduction buffers: a set for the draws (B rows) and one for the verify (B (gamma+1) rows + B gamma probes)
        self._draw = dict(red=torch.zeros(B, **i64), hi=torch.zeros((B, ops.HIST_BINS), **i64),
                          lo=torch.zeros((B, ops.HIST_BINS), **i64), cand=torch.zeros(B, **i64))
        self._verify = dict(red=torch.zeros(R + B * g, **i64), hi=torch.zeros((R, ops.HIST_BINS), **i64),
                            lo=torch.zeros((R, ops.HIST_BINS), **i64), cand=torch.zeros((B, ops.CAND_WORDS), **i64))

    def check_model(self, model):
        grp = getattr(model, "process_group", None)
        width = model.output.weight.shape[0]
        if grp is None:
            if not self.replicate_draft:
                raise ValueError("sharded sampling: the model is not tensor-parallel (an unsharded draft next to a sharded "
                                 "target needs replicate_draft=True; a one-GPU run takes the plain Sampler)")
            if width != self.vocab_total:
                raise ValueError(f"sharded sampling: the replicated draft's vocabulary ({width}) differs from the target's "
                                 f"({self.vocab_total})")
            return
        if grp is not self.group and not _same_ranks(grp, self.group):
            raise ValueError("sharded sampling: the model is sharded over another group of ranks than the sampler's "
                             f"({_group_ranks(grp)} vs {_group_ranks(self.group)}).  A draft sharded over a sub-group of the "
                             "target's ranks is not supported: the other ranks would have no draft ring to verify against")
        if width != self.v_loc:
            raise ValueError(f"sharded sampling: the model's local head width ({width}) differs from the sampler's "
                             f"({self.v_loc}); draft and target must shard equal vocabularies alike")

    def _reduce(self, t, op):
        dist.all_reduce(t, op=op, group=self.group)

    def _filter(self, logits, n, bufs, row_sel=None, tokens_buffer=None, ring=None, ring_col_offset=0):
        """Phases A-C: after it bufs holds the reduced max (+ probes) and histograms of the drawn rows."""
        T, p = self.temperature, self.top_p
        ops.shard_max(logits, n, self.vocab_offset, self.vocab_total, bufs["red"], row_sel=row_sel,
                      tokens_buffer=tokens_buffer, ring=ring, ring_col_offset=ring_col_offset)
        self._reduce(bufs["red"], dist.ReduceOp.MAX)
        ops.shard_hist(logits, n, T, p, bufs["red"], bufs["hi"], row_sel=row_sel)
        self._reduce(bufs["hi"], dist.ReduceOp.SUM)
        if p < 1:
            ops.shard_hist(logits, n, T, p, bufs["red"], bufs["lo"], hist_hi=bufs["hi"], row_sel=row_sel)
            self._reduce(bufs["lo"], dist.ReduceOp.SUM)
            return bufs["lo"]
        return None

    def head(self, logits, role, idx, B, n):
        T, p, s = self.temperature, self.top_p, self.seed
        if logits.shape[1] != self.v_loc:
            if role in ("draft", "prefill") and self.replicate_draft and logits.shape[1] == self.vocab_total:
                # the replicated draft (its prefill and its steps) holds whole rows on every rank: the one-GPU draw,
                # identical everywhere, counters included
                return super().head(logits, role, idx, B, n)
            raise ValueError(f"sharded sampling: {role} logits of width {logits.shape[1]}, this rank's is {self.v_loc}")
        if B != self.B:
            raise ValueError(f"sharded sampling: step of {B} requests, the sampler was built for {self.B}")
        if role == "verify":
            if n != self.gamma + 1:
                raise ValueError(f"verify step with {n} rows per request, sampler gamma = {self.gamma}")
            bufs = self._verify
            off = self.vocab_offset if self.replicate_draft else 0
            lo = self._filter(logits, 1, bufs, tokens_buffer=idx, ring=self.ring, ring_col_offset=off)
            ops.spec_verify_shard(logits, idx, self.vocab_offset, self.vocab_total, self.ring, self.ring_stats,
                                  bufs["red"], bufs["hi"], lo, self.target_stats, self.counters, T, p, s, bufs["cand"],
                                  ring_col_offset=off)
            self._reduce(bufs["cand"], dist.ReduceOp.MAX)
            return ops.spec_verify_shard_finish(bufs["cand"], idx, self.counters)
        if role == "draft":
            purpose, advance, draft = ops.SAMPLE_DRAFT, ops.ADVANCE_STEP, True
        elif role in ("prefill", "baseline"):
            purpose = ops.SAMPLE_PREFILL if role == "prefill" else ops.SAMPLE_BASELINE
            advance, draft = ops.ADVANCE_ITER, False
        else:
            raise ValueError(f"sampling: step role {role!r} is not one of {ROLES}")
        bufs = self._draw
        row_sel = self.row_sel if (draft and n == 2) else None
        lo = self._filter(logits, n, bufs, row_sel=row_sel)
        ops.shard_draw(logits, n, self.vocab_offset, self.vocab_total, T, p, s, purpose, self.counters, bufs["red"],
                       bufs["hi"], lo, bufs["cand"], row_sel=row_sel, ring=self.ring if draft else None,
                       ring_stats=self.ring_stats if draft else None)
        self._reduce(bufs["cand"], dist.ReduceOp.MAX)
        return ops.shard_finish(bufs["cand"], n, self.counters, advance)


def attach(backend, sampler):
    """Attach `sampler` (or None: greedy) to a back-end's model.  Switching drops the back-end's captured steps."""
    if backend is None:
        return
    model = backend.model
    if getattr(model, "sampler", None) is sampler:
        return
    if sampler is not None:
        sampler.check_model(model)
    from .graph import clear_graphs
    clear_graphs(backend)
    model.sampler = sampler
