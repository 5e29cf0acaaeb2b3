"""GPU tests of per-request sampling in the decode loops (Engine/sampling.RequestSampler): the five loops on the tiny
checkpoints.  Uniform parameters give the scalar Sampler's run, an all-greedy batch gives the greedy run, and in a mixed
batch (one greedy request, one sampled with top-k) every launch of the run is replayed through the scalar ops on
top-k-masked rows and matches bit for bit, the greedy request matching ops.argmax."""
import numpy as np
import pytest
import torch

from magicdec_amd import ops
from magicdec_amd.Engine.sampling import RequestSampler
from tests import golden_cfg as gc
from tests.test_gpu_engine import ckpt_dir  # noqa: F401  (fixture)
from tests.test_gpu_sampling import _stats_np
from tests.test_gpu_sampling_engine import LOOPS, T, TOP_P, _run
from tests.test_gpu_sampling_request import topk_mask

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIXED = ([0.0, 0.8], [1.0, 0.9], [0, 20])           # request 0 greedy; request 1 sampled, top-k 20 then top-p 0.9
assert gc.B == len(MIXED[0])


def _request_cls(temperature, top_p, top_k, cls=RequestSampler):
    """A stand-in for the `cls` of _run, which calls cls(T, TOP_P, seed, B, gamma, vocab, device)."""
    return lambda _t, _p, seed, B, gamma, vocab, dev: cls(temperature, top_p, top_k, seed, B, gamma, vocab, dev)


@pytest.mark.parametrize("loop", LOOPS)
def test_uniform_parameters_equal_the_scalar_sampler(loop, ckpt_dir):  # noqa: F811
    a, ta, _ = _run(loop, ckpt_dir, seed=5)
    b, tb, smp = _run(loop, ckpt_dir, seed=5, cls=_request_cls(T, TOP_P, 0))
    assert isinstance(smp, RequestSampler)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert ta == tb


@pytest.mark.parametrize("loop", LOOPS)
def test_an_all_greedy_batch_equals_the_greedy_run(loop, ckpt_dir):  # noqa: F811
    a, ta, _ = _run(loop, ckpt_dir, seed=None)
    b, tb, _ = _run(loop, ckpt_dir, seed=5, cls=_request_cls(0.0, 1.0, 0))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert ta == tb


class RecordingRequestSampler(RequestSampler):
    """RecordingSampler of tests/test_gpu_sampling_engine.py for the per-request form."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.log = []

    def head(self, logits, role, idx, B, n):
        rec = dict(role=role, n=n, B=B, logits=logits.clone(), before=self.counters.tolist(),
                   row_sel=self.row_sel.clone())
        if role == "verify":
            rec.update(tokens=idx.clone(), ring=self.ring.clone())
        out = super().head(logits, role, idx, B, n)
        rec.update(out=out.clone(), after=self.counters.tolist())
        if role == "draft":
            j = rec["before"][1]
            rec.update(slot=self.ring[:, j].clone(), slot_stats=self.ring_stats[:, j].clone())
        if role == "verify":
            rec["target_stats"] = self.target_stats.clone()
        self.log.append(rec)
        return out


def _m_z(st):
    m, _, z = _stats_np(st)
    return m, z


@pytest.mark.parametrize("loop", LOOPS)
def test_every_launch_of_a_mixed_batch_replays_through_the_scalar_ops(loop, ckpt_dir):  # noqa: F811
    _, _, smp = _run(loop, ckpt_dir, seed=9, cls=_request_cls(*MIXED, cls=RecordingRequestSampler))
    assert len(smp.log) > 3
    G = 0 if loop == "baseline" else gc.GAMMA
    V, seed, B = smp.vocab, smp.seed, gc.B
    (_, t1), (_, p1), (_, k1) = MIXED
    assert 1 <= k1 < V

    def masked(x):
        return topk_mask(x.cpu(), k1)[0].to(DEV)

    def counters(rec):
        return torch.tensor(rec["before"], dtype=torch.int32, device=DEV)

    ref_ring = torch.zeros((B, max(G, 1), V), dtype=torch.bfloat16, device=DEV)
    ref_rst = torch.zeros((B, max(G, 1), 2), dtype=torch.int64, device=DEV)
    count = dict(prefill=0, baseline=0, draft=0, verify=0)
    for rec in smp.log:
        role, n, lg, out = rec["role"], rec["n"], rec["logits"].contiguous(), rec["out"]
        count[role] += 1
        rows = lg.view(B, n, V)
        if role == "verify":
            assert n == G + 1
            assert torch.equal(out[0], ops.argmax(rows[0].contiguous())), "greedy request: target_tokens is not the argmax"
            assert torch.equal(masked(rec["ring"])[1], ref_ring[1])        # the replayed draws filled the same slots
            tst = torch.zeros((B * n, 2), dtype=torch.int64, device=DEV)
            ref = ops.spec_verify_sample(masked(lg), rec["tokens"], ref_ring, ref_rst, tst, counters(rec), t1, p1, seed)
            assert torch.equal(out[1], ref[1]), (rec["before"], out[1].tolist(), ref[1].tolist())
            mine, theirs = _m_z(rec["target_stats"].view(B, n, 2)[1]), _m_z(tst.view(B, n, 2)[1])
            assert np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1])
            continue
        sel = rec["row_sel"] if (role == "draft" and n == 2) else None
        pick = (sel - 1) if sel is not None else torch.full((B,), n - 1, device=DEV)
        drawn = rows[torch.arange(B, device=DEV), pick]
        assert bool((out == out[:, :1]).all())
        assert int(out[0, 0]) == int(ops.argmax(drawn[:1].contiguous())[0]), "greedy request: the draw is not the argmax"
        if role == "draft":
            assert torch.equal(rec["slot"], drawn), "the ring slot is not the unmasked selected row"
            ref = ops.sample_rows(masked(lg), n, t1, p1, seed, ops.SAMPLE_DRAFT, counters(rec), ops.ADVANCE_STEP,
                                  row_sel=sel, ring=ref_ring, ring_stats=ref_rst)
            j = rec["before"][1]
            mine, theirs = _m_z(rec["slot_stats"][1]), _m_z(ref_rst[1, j])
            assert np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1])
        else:
            purpose = ops.SAMPLE_PREFILL if role == "prefill" else ops.SAMPLE_BASELINE
            ref = ops.sample_rows(masked(lg), n, t1, p1, seed, purpose, counters(rec), ops.ADVANCE_ITER)
        assert torch.equal(out[1], ref[1]), (role, rec["before"], out[1].tolist(), ref[1].tolist())
    assert count["prefill"] >= 1
    if loop == "baseline":
        assert count["baseline"] > 3
    else:
        assert count["verify"] > 3 and count["draft"] == G * count["verify"]
