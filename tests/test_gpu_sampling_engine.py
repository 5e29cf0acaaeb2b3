"""GPU tests of temperature / top-p sampling in the decode loops (Engine/sampling.py): the five loops with a Sampler on
the tiny checkpoints -- same seed same output, hipGraph steps bit-identical to eager steps, another seed another
output, and every verify step's target_tokens reproduced by the numpy restatement (tests/sampling_ref.py) from the
exact logits and draft ring the kernels read."""
import numpy as np
import pytest
import torch

from magicdec_amd import harness
from magicdec_amd.Engine.sampling import Sampler
from tests import golden_cfg as gc
from tests import sampling_ref as sr
from tests.conftest import parity_report
from tests.test_gpu_engine import _hip, ckpt_dir  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, TOP_P = 0.8, 0.9
LOOPS = ["longspec_snapkv", "longspec_stream", "selfspec_snapkv", "selfspec_stream", "baseline"]


class RecordingSampler(Sampler):
    """Records what every verify launch read (eager runs only)."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.log = []

    def head(self, logits, role, idx, B, n):
        if role != "verify":
            return super().head(logits, role, idx, B, n)
        pre = dict(logits=logits.clone(), ring=self.ring.clone(), tokens=idx.clone(), iteration=int(self.counters[0]))
        out = super().head(logits, role, idx, B, n)
        pre["tt"] = out.clone()
        self.log.append(pre)
        return out


def _run(loop, ckpt_dir, seed, graphs=False, cls=Sampler):
    ids = gc.synthetic_batches()[1].to(DEV)
    if loop.startswith("longspec"):
        tgt = _hip("target", ckpt_dir)
        drf = _hip("snapkv_draft" if loop.endswith("snapkv") else "stream_draft", ckpt_dir)
        engines = (tgt, drf)
    elif loop.startswith("selfspec"):
        engines = (_hip("snapkv_self" if loop.endswith("snapkv") else "stream_self", ckpt_dir),)
    else:
        from magicdec_amd.Engine.SnapKV.backend import LMBackend
        from pathlib import Path
        e = LMBackend(dtype=torch.bfloat16, device=DEV)
        e.load_model(Path(ckpt_dir) / "tinytgt" / "model.pth", use_tp=False)
        e.setup_caches(max_batch_size=gc.B, max_seq_length=gc.MAX_LEN)
        engines = (e,)
    if graphs:
        for e in engines:
            e.compile()
    vocab = engines[0].model.output.weight.shape[0]
    smp = None if seed is None else cls(T, TOP_P, seed, gc.B, 0 if loop == "baseline" else gc.GAMMA, vocab, DEV)
    trace = []
    if loop.startswith("longspec"):
        st, _ = harness.run_longspec_batch(engines[0], engines[1], ids, gc.GAMMA, gc.MAX_LEN, gc.EOT_1, gc.EOT_2,
                                           trace_fn=lambda s: trace.append(s.accept_nums.tolist()), sampler=smp)
        out = (st.output.cpu(), st.num_nodes.cpu())
    elif loop.startswith("selfspec"):
        st, _ = harness.run_selfspec_batch(engines[0], ids, gc.GAMMA, gc.MAX_LEN, gc.EOT_1, gc.EOT_2,
                                           loop.endswith("stream"),
                                           trace_fn=lambda s: trace.append(s.accept_nums.tolist()), sampler=smp)
        out = (st.output.cpu(), st.num_nodes.cpu())
    else:
        o, steps, _ = harness.run_baseline_batch(engines[0], ids, ids.shape[1] + 48, gc.EOT_1, gc.EOT_2, sampler=smp)
        out = (o.cpu(),)
    return out, trace, smp


@pytest.mark.parametrize("loop", LOOPS)
def test_sampled_loop_is_seeded_deterministic_and_graph_identical(loop, ckpt_dir):  # noqa: F811
    a, ta, _ = _run(loop, ckpt_dir, seed=5)
    b, tb, _ = _run(loop, ckpt_dir, seed=5)
    c, tc, _ = _run(loop, ckpt_dir, seed=5, graphs=True)
    d, _, _ = _run(loop, ckpt_dir, seed=6)
    g, tg, _ = _run(loop, ckpt_dir, seed=None)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for x, y in zip(a, c):
        assert torch.equal(x, y), "hipGraph steps differ from eager steps"
    assert ta == tb == tc
    assert not torch.equal(a[0], d[0]), "another seed drew the same tokens"
    assert not torch.equal(a[0], g[0]), "the sampled run equals the greedy run"
    if ta:
        ah = np.mean([x for it in ta for x in it])
        ag = np.mean([x for it in tg for x in it])
        parity_report(f"[sampling] {loop}: mean accepted per iteration sampled (T={T}, top_p={TOP_P}) {ah:.3f} vs "
                      f"greedy {ag:.3f} (tiny random-init model; reported, not gated)")


@pytest.mark.parametrize("loop", LOOPS[:4])
def test_every_verify_step_matches_the_restatement(loop, ckpt_dir):  # noqa: F811
    _, _, smp = _run(loop, ckpt_dir, seed=9, cls=RecordingSampler)
    assert len(smp.log) > 3
    G = gc.GAMMA
    rows = diffs = 0
    for rec in smp.log:
        lg = rec["logits"].view(torch.int16).cpu().numpy().view(np.uint16)
        ring = rec["ring"].view(torch.int16).cpu().numpy().view(np.uint16)
        toks = rec["tokens"].cpu().numpy()
        tt = rec["tt"].cpu().numpy()
        B = toks.shape[0]
        for b in range(B):
            ref, fl = sr.verify(lg[b * (G + 1):(b + 1) * (G + 1)], ring[b], toks[b], T, TOP_P, smp.seed, b,
                                rec["iteration"])
            rows += 1
            if not np.array_equal(ref, tt[b]):
                assert fl, (b, ref.tolist(), tt[b].tolist())
                diffs += 1
    parity_report(f"[sampling] {loop}: {rows} verify rows vs restatement, {diffs} differ (all at flagged near-ties)")
