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
iteration.  TP = 1 only; one temperature / top_p per run (changing them after a capture needs clear_graphs()).
"""
from __future__ import annotations

import torch

from .. import ops

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
