"""Tensor-level wrappers of the per-request sampling entry points (include/magicdec_hip.h, K11 "per request").

The temperature, top_p and top_k of request b are element b of three device tensors the kernels read at launch time, so
a captured hipGraph serves every parameter change.  The operands shared with ops.sample_rows / ops.spec_verify_sample go
through the same contracts (ops._logits, ops._draft_ring, ...); the three parameter tensors are checked by dtype, shape
[B], device and contiguity only -- no value is read back to the host, the kernels map every out-of-range value to a
defined setting (T not > 0: greedy; top_p outside (0, 1): 1; top_k outside [1, vocab): off).
"""
from __future__ import annotations

import torch

from . import _lib, ops
from ._lib import check
from .ops import _p

F32 = torch.float32


def _request_params(what, temperature, top_p, top_k, B):
    for name, t in (("temperature", temperature), ("top_p", top_p), ("top_k", top_k)):
        if t is not None and not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a tensor of B = {B} values on the GPU, "
                            f"got {type(t).__name__}")
    ops._tensor(what, "temperature", temperature, (B,), F32)
    ops._tensor(what, "top_p", top_p, (B,), F32)
    ops._tensor(what, "top_k", top_k, (B,), ops.I32, optional=True)


def sample_rows_req(logits, n, temperature, top_p, top_k, seed, purpose, counters, advance, row_sel=None, ring=None,
                    ring_stats=None, out=None):
    """ops.sample_rows with request b's own temperature[b], top_p[b] (float32 [B]) and top_k[b] (int32 [B], or None:
    off).  A request whose temperature is not > 0 gets the row's argmax; in draft mode its row still goes to the
    ring."""
    B, vocab = ops._logits("sample_rows_req", logits, n=n, row_sel=row_sel)
    _request_params("sample_rows_req", temperature, top_p, top_k, B)
    ops._counters(counters)
    gamma = ops._draft_ring("sample_rows_req", ring, ring_stats, B, vocab)
    out = ops._tokens_out("sample_rows_req", out, B, n, logits.device)
    check(_lib.load().md_sample_rows_req(_p(logits), logits.stride(0), B, n, vocab, _p(temperature), _p(top_p),
                                         _p(top_k), int(seed) & 0xFFFFFFFFFFFFFFFF, int(purpose), _p(row_sel),
                                         _p(counters), int(advance), _p(ring), _p(ring_stats), gamma, _p(out),
                                         ops._stream()), "md_sample_rows_req")
    return out


def spec_verify_sample_req(logits, tokens_buffer, ring, ring_stats, target_stats, counters, temperature, top_p, top_k,
                           seed, out=None):
    """ops.spec_verify_sample with per-request parameters (see sample_rows_req).  A greedy request's target_tokens row
    is the argmax of each of its gamma + 1 target rows, what the greedy loop hands ops.accept_rollback."""
    rows, vocab = ops._logits("spec_verify_sample_req", logits)
    ops._counters(counters)
    B, G1, tb = ops._tokens_buffer("spec_verify_sample_req", tokens_buffer)
    _request_params("spec_verify_sample_req", temperature, top_p, top_k, B)
    if ring is None:
        raise ValueError("spec_verify_sample_req: ring is missing")
    ops._gpu(ring)
    if rows != B * G1 or tuple(ring.shape) != (B, G1 - 1, vocab) or ring.dtype != ops.BF16 or not ring.is_contiguous():
        raise ValueError(f"spec_verify_sample_req: logits {tuple(logits.shape)}, ring {tuple(ring.shape)} and "
                         f"tokens_buffer {tuple(tokens_buffer.shape)} disagree (draft and target vocabularies must be "
                         "equal)")
    ops._verify_stats("spec_verify_sample_req", target_stats, ring_stats, B, G1 - 1)
    out = ops._tokens_out("spec_verify_sample_req", out, B, G1, logits.device)
    check(_lib.load().md_spec_verify_sample_req(_p(logits), logits.stride(0), B, G1 - 1, vocab, _p(temperature),
                                                _p(top_p), _p(top_k), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(tb), _p(ring),
                                                _p(ring_stats), _p(target_stats), _p(counters), _p(out),
                                                ops._stream()), "md_spec_verify_sample_req")
    return out
