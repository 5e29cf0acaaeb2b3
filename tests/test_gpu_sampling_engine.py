"""GPU tests of temperature / top-p sampling in the decode loops (Engine/sampling.py): the five loops with a Sampler on
the tiny checkpoints -- same seed same output, hipGraph steps bit-identical to eager steps, another seed another
output, and every launch of a run (prefill, baseline, draft and verify draws) checked against the admissible-outcome
oracle of the numpy restatement (tests/sampling_ref.py) from the exact logits, ring, tokens and counters the kernels read."""
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
    """Records every launch (eager runs only): role, rows per request, the logits read, the row selector and the
    counters before the launch, the tokens returned, the counters after it; for a draft step the ring slot and stats it
    wrote; for a verify the tokens_buffer, ring and ring stats it read and the target stats it wrote."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.log = []

    def head(self, logits, role, idx, B, n):
        rec = dict(role=role, n=n, B=B, logits=logits.clone(), before=self.counters.tolist(),
                   row_sel=self.row_sel.cpu().clone())
        if role == "verify":
            rec.update(tokens=idx.clone(), ring=self.ring.clone(), ring_stats=self.ring_stats.clone())
        out = super().head(logits, role, idx, B, n)
        rec.update(out=out.clone(), after=self.counters.tolist())
        if role == "draft":
            j = rec["before"][1]
            rec.update(slot=self.ring[:, j].clone(), slot_stats=self.ring_stats[:, j].clone())
        if role == "verify":
            rec["target_stats"] = self.target_stats.clone()
        self.log.append(rec)
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


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _plain_draw_ok(bits, tok, seed, purpose, step, b, it):
    """A draw that wrote no statistics (prefill, baseline): admissible under one of the kstar values check_stats would
    accept (a plain draw reads nothing of the stats but the kept set)."""
    m, kstar, zk = sr.ref_stats(bits, T, TOP_P)
    _, allowed = sr._select(sr.key16(bits), np.exp(sr.exponents(bits, m, T)), TOP_P)
    sets = [sr.draw_admissible(sr.Row(bits, T, m, k, zk), seed, purpose, step, b, it) for k in sorted(allowed)]
    return any(tok in s for s in sets), max(len(s) for s in sets) > 1 or len(sets) > 1


@pytest.mark.parametrize("loop", LOOPS)
def test_every_verify_step_matches_the_restatement(loop, ckpt_dir):  # noqa: F811
    """Every launch of the run, not only the verify: each prefill, baseline and draft draw is an admissible draw of the
    restatement from the right ROW (the last one; row row_sel - 1 of the two-token draft step), with the right purpose,
    step index (draft step j: step j and ring slot j, slots filled 0..gamma-1 in order; everything else step 0) and
    iteration (one more per verify and per prefill / baseline draw); every verify's target_tokens is in the admissible
    set of the oracle computed from the logits, ring and tokens it read and the stats the kernels wrote."""
    from tests.test_gpu_sampling import _stats_np
    _, _, smp = _run(loop, ckpt_dir, seed=9, cls=RecordingSampler)
    assert len(smp.log) > 3
    G = 0 if loop == "baseline" else gc.GAMMA
    V, seed = smp.vocab, smp.seed
    it, step, two_token = 0, 0, 0
    count = dict(prefill=0, baseline=0, draft=0, verify=0)
    ambiguous = 0
    round_ = []                                           # the draft records of the running iteration
    want_sel, sel_seen = None, set()                      # row_sel the next two-token step must use; values it took
    for rec in smp.log:
        role, n, B = rec["role"], rec["n"], rec["B"]
        count[role] += 1
        lg = _bits(rec["logits"]).reshape(B, n, V)
        out = rec["out"].cpu().numpy()
        assert rec["before"] == [it, step, 0, 0], (role, rec["before"], it, step)
        if role in ("prefill", "baseline"):
            assert step == 0 and (out == out[:, :1]).all()
            purpose = sr.PREFILL if role == "prefill" else sr.BASELINE
            for b in range(B):
                ok, multi = _plain_draw_ok(lg[b, n - 1], out[b, 0], seed, purpose, 0, b, it)
                assert ok, (role, it, b, int(out[b, 0]))
                ambiguous += multi
            it += 1
            assert rec["after"] == [it, 0, 0, 0]
        elif role == "draft":
            assert step < G and n in (1, 2) and (out == out[:, :1]).all()
            two_token += n == 2
            assert n == 1 or step == 0
            sel = rec["row_sel"].numpy() if n == 2 else np.full(B, n)
            assert ((sel >= 1) & (sel <= n)).all()
            if n == 2:
                # independent of the sampler's own tensor: the accept loop's rule, from the previous verify launch
                # (the second row is the new one iff every draft of the request was accepted)
                assert want_sel is not None and np.array_equal(sel, want_sel), (it, sel.tolist(), want_sel.tolist())
                sel_seen.update(sel.tolist())
            slot, st = _bits(rec["slot"]), _stats_np(rec["slot_stats"])
            for b in range(B):
                row_bits = lg[b, sel[b] - 1]
                assert np.array_equal(slot[b], row_bits), (it, step, b, "ring slot is not the selected row")
                row = sr.check_stats(row_bits, T, TOP_P, *(a[b] for a in st), tag=f"{loop} draft it{it} step{step} b{b}")
                adm = sr.draw_admissible(row, seed, sr.DRAFT, step, b, it)
                assert out[b, 0] in adm, (it, step, b, int(out[b, 0]), adm)
                ambiguous += len(adm) > 1
            round_.append(rec)
            step += 1
            assert rec["after"] == [it, step, 0, 0]
        else:
            assert step == G and n == G + 1 and len(round_) == G
            toks, tt = rec["tokens"].cpu().numpy(), out
            ring = _bits(rec["ring"])
            rst, tst = _stats_np(rec["ring_stats"]), _stats_np(rec["target_stats"])
            for j, dr in enumerate(round_):
                assert torch.equal(rec["ring"][:, j], dr["slot"]) and torch.equal(rec["ring_stats"][:, j], dr["slot_stats"])
                assert np.array_equal(toks[:, j + 1], dr["out"][:, 0].cpu().numpy())
            for b in range(B):
                rrows = [sr.check_stats(ring[b, j], T, TOP_P, *(a[b * G + j] for a in rst)) for j in range(G)]
                trows = [sr.check_stats(lg[b, j], T, TOP_P, *(a[b * (G + 1) + j] for a in tst)) for j in range(G + 1)]
                outs = sr.verify_admissible(trows, rrows, toks[b], seed, b, it)
                assert sr.contains(outs, tt[b]), (it, b, tt[b].tolist(), [o.tolist() for o in outs[:8]])
                ambiguous += len(outs) > 1
            full = (tt[:, :G] == toks[:, 1:]).all(axis=1) & ~np.isin(toks[:, 1:], (gc.EOT_1, gc.EOT_2)).any(axis=1)
            want_sel = np.where(full, 2, 1)
            it, step, round_ = it + 1, 0, []
            assert rec["after"] == [it, 0, 0, 0]
    assert count["prefill"] >= 1
    if loop == "baseline":
        assert count["baseline"] > 3 and count["draft"] == count["verify"] == 0
    else:
        assert count["verify"] > 3 and count["draft"] == G * count["verify"]
    if loop in ("longspec_snapkv", "longspec_stream", "selfspec_stream"):
        assert two_token >= 1, "no two-token draft step (row_sel) occurred in this run"
        assert 2 in sel_seen
    parity_report(f"[sampling] {loop}: {count['prefill']} prefill, {count['baseline']} baseline, {count['draft']} draft "
                  f"({two_token} two-token) and {count['verify']} verify launches vs the oracle: row, purpose, step, slot "
                  f"and iteration of every draw; {ambiguous} draws / verify rows with more than one admissible outcome, "
                  f"0 outside the admissible set")
