"""End-to-end GPU parity of the Engine back-ends and the decode loops against the oracle (run with -m gpu).

Method: the oracle (CPU) runs the reference's loop on a tiny GQA model; every Engine call it makes is recorded
(inputs, state before/after, output tokens, its logits).  The SAME call sequence is then replayed with
teacher-forced inputs and states on (a) the HIP back-ends and (b) THREE yardstick CPU oracles, each another valid
implementation of the reference's bf16 arithmetic: linears evaluated in float64 and rounded once
(oracle.magicdec_ref.LINEAR_MODE = "fp64": another summation order), the attention's probabilities rounded to bf16 before
the P.V product (oracle.flashinfer_ref.ATTN_P_MODE = "bf16": the tensor-core algorithm flashinfer's kernels and
csrc/attn.hip run), and both together.  Per call:
  * integer state (cachelens, last_page_len, indptr, draft twins): bit-exact;
  * logits: the measured gate  err_hip <= 2 * err_alt + 2 bf16 ulp  where err_x = max |x - oracle| over the call, alt =
    the float64-linear oracle, and the ulp is taken at the call's largest |logit|;
  * tokens: identical, except where the oracle's own top-2 gap is below twice that gate (an argmax that the allowed
    logit error can legitimately flip); every such flip is counted, the yardsticks' own flips are counted beside it
    (round 5: the bf16-P oracle alone flips as many as the HIP engine or more), and the HIP count is gated against them
    (flip_gate).  On peaked logits (a tiny pair, and a pair with the REAL layer widths and batch of configs[2]) no token
    may differ at all.
All measured errors go to the parity report (tests/conftest.py).
A second test runs the free-running HIP loop (no teacher forcing) and checks the speculative-decoding invariant: its
output equals the HIP autoregressive output token for token, diverging only at a logged near-tie.
"""
import os
import tempfile

import pytest
import torch

from oracle import harness_ref as hr
from oracle import magicdec_ref as mr
from tests import golden_cfg as gc
from tests.conftest import parity_report
from tests.parity_util import capped_threads

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _capped_cpu_threads():
    """The oracle runs of these tests are yardsticks behind tolerance gates (tokens within the measured logit gate,
    integer state teacher-forced), never bit-compared with the GPU: cap torch's intra-op pool, which on the GPU boxes'
    256-core hosts makes the small CPU matmuls of the oracle tens of times slower (tests/parity_util.capped_threads)."""
    from tests.parity_util import capped_threads
    with capped_threads():
        yield
DEV = "cuda:0"
# err_hip <= GATE_FACTOR * err_alt + GATE_ULPS * ulp_bf16(max |logit|).  Two ulps: one for the final bf16 rounding of
# the logits, one for what the float64-linear oracle does NOT model -- the attention kernel multiplies P in bf16
# (the tensor-core algorithm, bound in tests/parity_util.py) and RMSNorm / SiLU are gated at 1 ulp (test_gpu_ops.py).
GATE_FACTOR, GATE_ULPS = 2.0, 2.0
STATE = ("cachelens", "paged_kv_last_page_len", "paged_kv_indptr", "draft_cachelens", "draft_paged_kv_last_page_len",
         "draft_paged_kv_indptr")
MUT = ("cachelens", "paged_kv_last_page_len", "draft_cachelens", "draft_paged_kv_last_page_len")


def _ulp_at(x):
    """bf16 spacing at magnitude x (float)."""
    import math
    return 2.0 ** (math.floor(math.log2(max(abs(x), 2.0 ** -126))) - 7)


@pytest.fixture(scope="module")
def ckpt_dir():
    """Checkpoints of the tiny configs under <tmp>/<name>/model.pth + the configs registered by name."""
    from magicdec_amd.Engine import model_core
    d = tempfile.mkdtemp(prefix="md_ckpt_")
    for name in gc.TINY:
        cfg, sd = gc.tiny(name)
        os.makedirs(os.path.join(d, name), exist_ok=True)
        torch.save(sd, os.path.join(d, name, "model.pth"))
        model_core.transformer_configs[name] = gc.config_kwargs(cfg)
    return d


class Recorder:
    """Wraps a RefEngine: records every public call with state before/after and the oracle's logits."""

    def __init__(self, eng, tag, log):
        self.eng, self.tag, self.log = eng, tag, log

    def __getattr__(self, name):
        attr = getattr(self.eng, name)
        if name not in ("encode", "draft_encode", "inference", "verify", "speculate"):
            return attr

        def call(*a, **kw):
            pre = {k: getattr(self.eng, k).clone() for k in STATE if getattr(self.eng, k, None) is not None}
            out = attr(*a, **kw)
            post = {k: getattr(self.eng, k).clone() for k in STATE if getattr(self.eng, k, None) is not None}
            ids = a[0] if a else kw["input_ids"]
            lg = self.eng.model.last_logits.float()
            rec = dict(tag=self.tag, fn=name, ids=ids.clone(), cu=kw.get("cachelen_update"), out=out.clone(),
                       pre=pre, post=post, logits=lg.clone())
            if getattr(self.eng, "kv_fp8", False) and name == "encode":
                rec["kv_scales"] = [(ks.clone(), vs.clone()) for ks, vs in self.eng.kv_scales]
            self.log.append(rec)
            return out
        return call

    def __setattr__(self, k, v):
        if k in ("eng", "tag", "log"):
            object.__setattr__(self, k, v)
        else:
            setattr(self.eng, k, v)


class Stats:
    def __init__(self):
        self.npos = self.nties = self.nties_alt = self.nties_p = self.nties_both = self.calls = 0
        self.err_hip = self.err_alt = self.err_p = self.err_both = self.worst_ratio = 0.0

    def line(self, tag):
        return (f"[lockstep] {tag:34s} calls={self.calls:4d} positions={self.npos:6d} argmax flips vs the oracle: hip="
                f"{self.nties:3d} fp64-linear oracle={self.nties_alt:3d} bf16-P oracle={self.nties_p:3d} "
                f"fp64-linear+bf16-P oracle={self.nties_both:3d}  max|hip-oracle|={self.err_hip:.4f}  "
                f"max|fp64oracle-oracle|={self.err_alt:.4f}  max|bf16P-oracle|={self.err_p:.4f}  "
                f"max|fp64+bf16P-oracle|={self.err_both:.4f}  worst err_hip/gate={self.worst_ratio:.3f}")


# Flip-count gate.  The HIP attention runs the tensor-core algorithm (P rounded to bf16 before the
# P.V product, as flashinfer's kernels do); rounds 2-4 ASSERTED that this explains why the HIP engine flips more
# near-tie argmaxes than the float64-linear yardstick.  Now it is measured: the bf16-P oracle ALONE flips 18-20 of
# ~1 000-1 700 positions where the float64-linear one flips 6-13 and the HIP engine 15-18 (tools/lockstep_yardsticks.py
# on the CPU; profiles/r05_parity_report.txt on the GPU box).  Gate: the HIP count may exceed the larger of the two
# bf16-P yardsticks by 3 plus one standard deviation of a count of that size (two valid implementations are two draws of
# the same near-tie lottery; the oracle's own log differs from host to host).
def flip_gate(n_p, n_both):
    y = max(n_p, n_both)
    return y + 3 + y ** 0.5


def _oracle_call(eng, rec, linear_mode, p_mode):
    """One recorded call on a CPU oracle engine under the given arithmetic modes; returns (tokens, logits)."""
    from oracle import flashinfer_ref as fr
    for k in MUT:
        if k in rec["pre"] and getattr(eng, k, None) is not None:
            setattr(eng, k, rec["pre"][k].clone())
    if "kv_scales" in rec:
        eng.kv_scale_override = rec["kv_scales"]
    kwa = {}
    if rec["cu"] is not None:
        kwa["cachelen_update"] = rec["cu"].clone()
    mr.LINEAR_MODE, fr.ATTN_P_MODE = linear_mode, p_mode
    try:
        with capped_threads():          # the yardsticks only; the oracle's own run keeps torch's default
            out = getattr(eng, rec["fn"])(rec["ids"].clone(), **kwa)
    finally:
        mr.LINEAR_MODE, fr.ATTN_P_MODE = "fp32", "fp32"
    for k, v in rec["post"].items():
        assert getattr(eng, k).tolist() == v.tolist(), ("yardstick oracle", linear_mode, p_mode, rec["tag"], rec["fn"], k)
    return out, eng.model.last_logits.float()


def replay(log, engines, alt_engines):
    """Replays the oracle's call log on the HIP back-ends and on three yardstick oracles -- float64 linears (another
    summation order), bf16 P in the attention's P.V product (the tensor-core algorithm; oracle.flashinfer_ref
    .ATTN_P_MODE), and both together (the arithmetic class the HIP engine belongs to); gates per call.  `engines` may
    be None: the yardsticks alone (CPU), used by tools/lockstep_yardsticks.py."""
    import copy
    st = Stats()
    yard = alt_engines is not None               # None: no yardstick oracles (full-width models: float64 linears of a
    #                                              128 256-row head cost seconds per call) -- a fixed 4-ulp logit gate
    if yard:
        p_engines = copy.deepcopy(alt_engines)       # fresh engines: same weights, empty caches
        both_engines = copy.deepcopy(alt_engines)
    for rec in log:
        ref = rec["logits"]
        want = rec["out"]
        st.calls += 1
        st.npos += want.numel()
        err_alt = None
        if yard:
            a = alt_engines[rec["tag"]]
            out_alt, la = _oracle_call(a, rec, "fp64", "fp32")
            out_p, lp = _oracle_call(p_engines[rec["tag"]], rec, "fp32", "bf16")
            out_both, lb = _oracle_call(both_engines[rec["tag"]], rec, "fp64", "bf16")
            err_alt = (la.view(ref.shape) - ref).abs().max().item()
            st.err_alt = max(st.err_alt, err_alt)
            st.err_p = max(st.err_p, (lp.view(ref.shape) - ref).abs().max().item())
            st.err_both = max(st.err_both, (lb.view(ref.shape) - ref).abs().max().item())
            # the yardsticks' own flips: valid implementations of the same bf16 arithmetic also land on the other side
            # of the oracle's near-ties
            st.nties_alt += int((out_alt.view(want.shape) != want).sum())
            st.nties_p += int((out_p.view(want.shape) != want).sum())
            st.nties_both += int((out_both.view(want.shape) != want).sum())
        if engines is None:
            continue
        e = engines[rec["tag"]]
        for k in MUT:
            if k in rec["pre"] and getattr(e, k, None) is not None:
                setattr(e, k, rec["pre"][k].clone().to(DEV))
        if "kv_scales" in rec:      # fp8 cache: all replays quantise with the oracle's static scales
            e.model.kv_scale_override = [(ks.to(DEV), vs.to(DEV)) for ks, vs in rec["kv_scales"]]
        kw = {}
        if rec["cu"] is not None:
            kw["cachelen_update"] = rec["cu"].to(DEV)
        out = getattr(e, rec["fn"])(rec["ids"].to(DEV), **kw).cpu()
        for k, v in rec["post"].items():
            assert getattr(e, k).cpu().tolist() == v.tolist(), (rec["tag"], rec["fn"], k)
        lg = e.model._last_logits.float().cpu().view(ref.shape)
        err_hip = (lg - ref).abs().max().item()
        gate = (GATE_FACTOR * err_alt + GATE_ULPS * _ulp_at(ref.abs().max().item()) if yard
                else 4.0 * _ulp_at(ref.abs().max().item()))
        st.err_hip = max(st.err_hip, err_hip)
        st.worst_ratio = max(st.worst_ratio, err_hip / gate)
        assert err_hip <= gate, (rec["tag"], rec["fn"], f"err_hip {err_hip:.5f} > gate {gate:.5f} (err_alt {err_alt})")
        assert out.shape == want.shape
        neq = out != want
        if neq.any():
            # an argmax the allowed logit error can flip: the ORACLE's logit of our token within 2*gate of its maximum
            olg = ref.view(-1, ref.shape[-1])
            ours = olg.gather(1, out.view(-1, 1)).view(want.shape)
            best = olg.max(dim=-1).values.view(want.shape)
            ok = (best - ours) <= 2 * gate
            assert bool(ok[neq].all()), (rec["tag"], rec["fn"], out[neq], want[neq], (best - ours)[neq], gate)
            st.nties += int(neq.sum())
    # Bound on the COUNT (each single flip was already required to sit inside the oracle's own near-tie gap): against
    # the bf16-P yardsticks, see flip_gate (rounds 2-4: hip <= 2 x float64-linear + 6).  All four counts are in every
    # [lockstep] line of the parity report.  On peaked distributions all counts are zero
    # (test_peaked_logits_lockstep_has_zero_token_flips).
    assert not yard or st.nties <= flip_gate(st.nties_p, st.nties_both), \
        (f"hip flipped {st.nties} argmaxes vs the oracle; yardsticks: float64-linear {st.nties_alt}, bf16-P "
         f"{st.nties_p}, both {st.nties_both} (gate {flip_gate(st.nties_p, st.nties_both):.1f}): a kernel carries a bias")
    return st


def _alt(mode, cfg, sd, B, max_len=0, budget=0, **kw):
    return mr.RefEngine(mode, cfg, sd, B, max_len, budget, **kw)


def _hip(kind, ckpt_dir):
    from pathlib import Path
    p = lambda n: Path(ckpt_dir) / n / "model.pth"
    if kind == "target":
        from magicdec_amd.Engine.SnapKV.backend import LMBackend
        e = LMBackend(dtype=torch.bfloat16, device=DEV, dec_len=gc.GAMMA + 1)
        e.load_model(p("tinytgt"), use_tp=False)
        e.setup_caches(max_batch_size=gc.B, max_seq_length=gc.MAX_LEN)
    elif kind in ("snapkv_draft", "snapkv_draft_rej"):
        from magicdec_amd.Engine.SnapKV.backend_draft import LMBackend_Draft
        e = LMBackend_Draft(dtype=torch.bfloat16, device=DEV, draft_budget=gc.BUDGET)
        e.load_model(p("tinydrf" if kind.endswith("rej") else "tinytgt"), use_tp=False)
        e.setup_caches(max_batch_size=gc.B, max_seq_length=gc.MAX_LEN, draft_budget=gc.BUDGET)
    elif kind == "stream_draft":
        from magicdec_amd.Engine.StreamingLLM.backend_draft import LMBackend_Draft
        e = LMBackend_Draft(dtype=torch.bfloat16, device=DEV)
        e.load_model(p("tinytgt"), use_tp=False)
        e.setup_caches(max_batch_size=gc.B, draft_budget=gc.BUDGET)
    elif kind == "snapkv_self":
        from magicdec_amd.Engine.SnapKV.backend import LMBackend
        e = LMBackend(dtype=torch.bfloat16, device=DEV, dec_len=gc.GAMMA + 1, draft_dec_len=1)
        e.load_model(p("tinytgt"), use_tp=False)
        e.setup_caches(max_batch_size=gc.B, max_seq_length=gc.MAX_LEN, draft_budget=gc.BUDGET)
    elif kind == "stream_self":
        from magicdec_amd.Engine.StreamingLLM.backend import LMBackend
        e = LMBackend(dtype=torch.bfloat16, device=DEV, dec_len=gc.GAMMA + 1)
        e.load_model(p("tinytgt"), use_tp=False)
        e.setup_caches(max_batch_size=gc.B, max_seq_length=gc.MAX_LEN, draft_budget=gc.BUDGET)
    else:
        raise KeyError(kind)
    return e


N_BATCH = 2


@pytest.mark.parametrize("draft_kind", ["snapkv_draft", "stream_draft"])
def test_longspec_lockstep_with_oracle(draft_kind, ckpt_dir):
    cfg, sd = gc.tiny("tinytgt")
    log = []
    tgt = Recorder(mr.RefEngine("target", cfg, sd, gc.B, gc.MAX_LEN), "T", log)
    if draft_kind == "snapkv_draft":
        drf = Recorder(mr.RefEngine("snapkv_draft", cfg, sd, gc.B, gc.MAX_LEN, gc.BUDGET), "D", log)
    else:
        drf = Recorder(mr.RefEngine("stream_draft", cfg, sd, gc.B, 0, gc.BUDGET), "D", log)
    for ids in gc.synthetic_batches()[:N_BATCH]:
        hr.longspec_batch(tgt, drf, ids, gc.GAMMA, gc.MAX_LEN, gc.EOT_1, gc.EOT_2)
    alt = {"T": _alt("target", cfg, sd, gc.B, gc.MAX_LEN),
           "D": (_alt("snapkv_draft", cfg, sd, gc.B, gc.MAX_LEN, gc.BUDGET) if draft_kind == "snapkv_draft"
                 else _alt("stream_draft", cfg, sd, gc.B, 0, gc.BUDGET))}
    st = replay(log, {"T": _hip("target", ckpt_dir), "D": _hip(draft_kind, ckpt_dir)}, alt)
    parity_report(st.line(f"longspec/{draft_kind}"))


@pytest.mark.parametrize("kind", ["snapkv_self", "stream_self"])
def test_selfspec_lockstep_with_oracle(kind, ckpt_dir):
    cfg, sd = gc.tiny("tinytgt")
    log = []
    eng = Recorder(mr.RefEngine(kind, cfg, sd, gc.B, gc.MAX_LEN, gc.BUDGET), "T", log)
    for ids in gc.synthetic_batches()[:N_BATCH]:
        hr.selfspec_batch(eng, ids, gc.GAMMA, gc.MAX_LEN, gc.EOT_1, gc.EOT_2, kind == "stream_self")
    st = replay(log, {"T": _hip(kind, ckpt_dir)}, {"T": _alt(kind, cfg, sd, gc.B, gc.MAX_LEN, gc.BUDGET)})
    parity_report(st.line(f"selfspec/{kind}"))


def test_hip_loop_equals_hip_autoregressive(ckpt_dir):
    """Greedy speculative decoding must reproduce greedy autoregressive decoding (same engine, same kernels):
    free-running HIP longspec loop vs HIP baseline loop on the same prompts, token for token.  The verify pass scores
    gamma+1 rows at once and the baseline one row (different GEMM shapes -> hipBLASLt kernels -> summation orders), so
    the two may part ways ONLY where the baseline's own logits nearly tie: at the first differing token of a sequence
    the baseline's logit gap between its token and the speculative run's token must be <= 4 bf16 ulps at the logit
    scale (2 ulps of error on either side).  Every divergence is logged; after it the two sequences have different
    contexts and are not compared further."""
    from magicdec_amd import harness
    tgt, drf = _hip("target", ckpt_dir), _hip("stream_draft", ckpt_dir)
    ids = gc.synthetic_batches()[0].to(DEV)
    st, _ = harness.run_longspec_batch(tgt, drf, ids, gc.GAMMA, gc.MAX_LEN, gc.EOT_1, gc.EOT_2)
    spec_out, spec_n = st.output.cpu(), st.num_nodes.cpu()
    # baseline with its per-step logits kept: step t (0 = prefill) produced generated token t
    step_logits = []
    enc, inf = tgt.encode, tgt.inference

    def rec_encode(*a, **k):
        out = enc(*a, **k)
        step_logits.append(tgt.model._last_logits.float().view(gc.B, -1, tgt.model._last_logits.shape[-1])[:, -1].cpu())
        return out

    def rec_inference(*a, **k):
        out = inf(*a, **k)
        step_logits.append(tgt.model._last_logits.float().view(gc.B, -1, tgt.model._last_logits.shape[-1])[:, -1].cpu())
        return out
    tgt.encode, tgt.inference = rec_encode, rec_inference
    try:
        base_out, steps, _ = harness.run_baseline_batch(tgt, ids, gc.MAX_LEN, -1, -1)
    finally:
        tgt.encode, tgt.inference = enc, inf
    base_out = base_out.cpu()
    agree = total = ndiv = 0
    for b in range(gc.B):
        n = min(int(spec_n[b]), base_out.shape[1])
        a, c = spec_out[b, gc.S:n], base_out[b, gc.S:n]
        neq = torch.nonzero(a != c)
        total += len(a)
        if len(neq) == 0:
            agree += len(a)
            continue
        t = int(neq[0])
        agree += t
        ndiv += 1
        lg = step_logits[t][b]
        gap = (lg[int(c[t])] - lg[int(a[t])]).item()
        ulp = _ulp_at(lg.abs().max().item())
        parity_report(f"[spec == autoregressive] seq {b}: diverges at generated token {t}: baseline token {int(c[t])} "
                      f"vs speculative {int(a[t])}, baseline logit gap {gap:.5f} = {gap / ulp:.2f} bf16 ulp")
        assert 0 <= gap <= 4 * ulp, f"seq {b} token {t}: divergence at a logit gap of {gap / ulp:.2f} ulp"
    parity_report(f"[spec == autoregressive] agreeing prefix {agree}/{total} generated tokens, {ndiv} near-tie "
                  f"divergences, iterations={st.iters}")
    assert st.iters > 0 and total > 0


# case -> (the _hip kinds of its engines, the reference trace of the same loop on the same tiny models, if the loop has
# a two-token step)
HIPGRAPH_CASES = {
    "longspec/snapkv_draft": (("target", "snapkv_draft"), "run_longspec_snapkv.json"),
    "longspec/stream_draft": (("target", "stream_draft"), "run_longspec_stream.json"),
    "snapkv_self": (("snapkv_self",), None),
    "stream_self": (("stream_self",), "run_selfspec_stream.json"),
}
HIPGRAPH_BATCH = 1      # of gc.synthetic_batches(): the reference's own traces show two-token steps in it (checked below)


def _reference_two_token_steps(golden, batch):
    """cachelen_update records of batch `batch` in a committed reference trace (a batch starts with the first call's kind)."""
    trace = gc.load_json(golden)["trace"]
    first, b, n = (trace[0]["cls"], trace[0]["fn"]), -1, 0
    for r in trace:
        b += (r["cls"], r["fn"]) == first
        n += b == batch and "cachelen_update" in r
    return n


@pytest.mark.parametrize("case", list(HIPGRAPH_CASES))
def test_hipgraph_steps_equal_eager_steps(case, ckpt_dir):
    """engine.compile() (hipGraph capture of the decode steps, Engine/graph.py) must not change a single token or
    length: each free-running loop with graphs == without graphs, bit for bit (same kernels, deterministic) -- output,
    num_nodes, the accept trace and every length / last-page tensor of every engine.  Every loop that has one must run
    its two-token step (after an all-accept iteration) under graphs: that step REBINDS the last-page length it advanced
    (`cachelen_update`), which a captured step that does not pin every tensor it reads would miss."""
    from magicdec_amd import harness
    kinds, golden = HIPGRAPH_CASES[case]
    assert golden is None or _reference_two_token_steps(golden, HIPGRAPH_BATCH) > 0
    ids = gc.synthetic_batches()[HIPGRAPH_BATCH].to(DEV)
    outs = []
    for use_graphs in (False, True):
        engines = [_hip(k, ckpt_dir) for k in kinds]
        if use_graphs:
            for e in engines:
                e.compile()
        trace = []
        kw = dict(trace_fn=lambda s: trace.append(s.accept_nums.tolist()))
        if len(engines) == 2:
            st, _ = harness.run_longspec_batch(*engines, ids, gc.GAMMA, gc.MAX_LEN, gc.EOT_1, gc.EOT_2, **kw)
        else:
            st, _ = harness.run_selfspec_batch(engines[0], ids, gc.GAMMA, gc.MAX_LEN, gc.EOT_1, gc.EOT_2,
                                               case == "stream_self", **kw)
        assert not use_graphs or all(e._use_graphs and e._graphs for e in engines), "a capture fell back to eager"
        state = [getattr(e, k).cpu() for e in engines for k in MUT if getattr(e, k, None) is not None]
        outs.append((trace, [st.output.cpu(), st.num_nodes.cpu()] + state))
    (trace_a, a), (trace_b, b) = outs
    assert trace_a == trace_b and len(trace_a) > 3, "accept traces differ"
    assert len(a) == len(b) >= 2 + 2 * len(kinds)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    if golden is not None:      # an all-accept iteration that was not the last: the next one began with the two-token step
        assert any(max(acc) == gc.GAMMA + 1 for acc in trace_b[:-1]), trace_b


# ------------------------------------------------------------------ other model families of the reference's zoo
EXTRA = {
    # Qwen2.5-style: qkv bias, g = 5 (padded MFMA M tile, mis-aligned SnapKV mask), eps 1e-6, plain RoPE theta 1e6
    "tinyqwen": dict(cfg=mr.RefConfig(n_layer=2, n_head=10, n_local_heads=2, dim=640, intermediate_size=1280,
                                      vocab_size=2048, rope_base=1000000.0, norm_eps=1e-6, qkv_bias=True), seed=21),
    # Llama-3.1-70B-style: g = 8 -> two MFMA M tiles per (request, kv head) in the verify kernel, D = 128
    "tiny70b": dict(cfg=mr.RefConfig(n_layer=2, n_head=16, n_local_heads=2, dim=2048, intermediate_size=2048,
                                     vocab_size=2048, rope_base=500000.0, scaling_factor=8, high_freq_factor=4,
                                     low_freq_factor=1, original_max_position_embeddings=8192), seed=22),
    # llama-68m (BASELINE configs[0]): MHA g = 1, D = 64, vocab 32000
    "tiny68m": dict(cfg=mr.RefConfig(n_layer=2, n_head=12, n_local_heads=12, dim=768, intermediate_size=3072,
                                     vocab_size=32000), seed=23),
}


def _extra_ckpt(name):
    from pathlib import Path
    from magicdec_amd.Engine import model_core
    e = EXTRA[name]
    cfg = e["cfg"]
    sd = mr.init_state_dict(cfg, e["seed"], wo_scale=0.1)
    d = tempfile.mkdtemp(prefix="md_ckpt_")
    os.makedirs(os.path.join(d, name))
    torch.save(sd, os.path.join(d, name, "model.pth"))
    model_core.transformer_configs[name] = dict(
        block_size=4096, n_layer=cfg.n_layer, n_head=cfg.n_head, n_local_heads=cfg.n_local_heads, dim=cfg.dim,
        intermediate_size=cfg.intermediate_size, vocab_size=cfg.vocab_size, rope_base=cfg.rope_base,
        norm_eps=cfg.norm_eps, scaling_factor=cfg.scaling_factor, high_freq_factor=cfg.high_freq_factor,
        low_freq_factor=cfg.low_freq_factor, original_max_position_embeddings=cfg.original_max_position_embeddings,
        qkv_bias=cfg.qkv_bias)
    return cfg, sd, Path(d) / name / "model.pth"


def test_peaked_logits_lockstep_has_zero_token_flips():
    """north_star's "accepted-token sequences identical", literally: on a target / draft pair with PEAKED next-token
    distributions (tests/golden_cfg.py:peaked_pair -- what trained checkpoints have; the random-init tiny models of the
    other lock-step tests have ~2048 nearly tied logits, where their measured gate has to tolerate near-tie flips) the
    HIP engines must reproduce EVERY token of EVERY call of the oracle's longspec run: zero flips over >= 1000
    positions, with the oracle's own top-2 gap >= 16 bf16 ulps on >= 99 % of them (asserted, so the zero is
    meaningful).  The draft mispredicts a quarter of the token ids, so rejections / rollbacks / bonus tokens are in
    the run; logits still pass the measured gate of the other tests."""
    from pathlib import Path
    from magicdec_amd.Engine import model_core
    from magicdec_amd.Engine.SnapKV.backend import LMBackend
    from magicdec_amd.Engine.SnapKV.backend_draft import LMBackend_Draft
    (cfg_t, sd_t), (cfg_d, sd_d) = gc.peaked_pair()
    d = tempfile.mkdtemp(prefix="md_ckpt_")
    for name, cfg, sd in (("peakedtgt", cfg_t, sd_t), ("peakeddrf", cfg_d, sd_d)):
        os.makedirs(os.path.join(d, name))
        torch.save(sd, os.path.join(d, name, "model.pth"))
        model_core.transformer_configs[name] = gc.config_kwargs(cfg)
    log = []
    tgt = Recorder(mr.RefEngine("target", cfg_t, sd_t, gc.B, gc.MAX_LEN), "T", log)
    drf = Recorder(mr.RefEngine("snapkv_draft", cfg_d, sd_d, gc.B, gc.MAX_LEN, gc.BUDGET), "D", log)
    iters = 0
    for ids in gc.synthetic_batches()[:3]:
        iters += hr.longspec_batch(tgt, drf, ids, gc.GAMMA, gc.MAX_LEN, gc.EOT_1, gc.EOT_2)["iters"]
    # how peaked the oracle's distributions are, over the positions of every recorded call
    npos = wide = 0
    for rec in log:
        lg = rec["logits"].view(-1, rec["logits"].shape[-1])
        top2 = lg.topk(2, dim=-1).values
        ulp = torch.tensor([_ulp_at(float(v)) for v in top2[:, 0]])
        npos += lg.shape[0]
        wide += int(((top2[:, 0] - top2[:, 1]) >= 16 * ulp).sum())
    assert npos >= 1000 and wide >= 0.99 * npos, (npos, wide)
    generated = sum(r["out"].numel() for r in log if r["tag"] == "T" and r["fn"] == "inference")
    e_t = LMBackend(dtype=torch.bfloat16, device=DEV, dec_len=gc.GAMMA + 1)
    e_t.load_model(Path(d) / "peakedtgt" / "model.pth", use_tp=False)
    e_t.setup_caches(max_batch_size=gc.B, max_seq_length=gc.MAX_LEN)
    e_d = LMBackend_Draft(dtype=torch.bfloat16, device=DEV, draft_budget=gc.BUDGET)
    e_d.load_model(Path(d) / "peakeddrf" / "model.pth", use_tp=False)
    e_d.setup_caches(max_batch_size=gc.B, max_seq_length=gc.MAX_LEN, draft_budget=gc.BUDGET)
    alt = {"T": _alt("target", cfg_t, sd_t, gc.B, gc.MAX_LEN),
           "D": _alt("snapkv_draft", cfg_d, sd_d, gc.B, gc.MAX_LEN, gc.BUDGET)}
    st = replay(log, {"T": e_t, "D": e_d}, alt)
    parity_report(st.line("longspec/peaked-logits") + f"  | top-2 gap >= 16 ulp on {wide}/{npos} positions, "
                  f"{iters} iterations, {generated} verify positions")
    assert st.nties == 0, f"{st.nties} tokens differ from the oracle's on peaked distributions"
    assert st.npos >= 1000


@pytest.mark.parametrize("name", ["tinyqwen", "tiny70b"])
def test_selfspec_snapkv_lockstep_other_families(name):
    """Self-speculation with a SnapKV draft cache (configs[4] style) on Qwen-like (g=5, bias) and 70B-like (g=8)."""
    from magicdec_amd.Engine.SnapKV.backend import LMBackend
    cfg, sd, ck = _extra_ckpt(name)
    log = []
    eng = Recorder(mr.RefEngine("snapkv_self", cfg, sd, gc.B, gc.MAX_LEN, gc.BUDGET), "T", log)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(4, cfg.vocab_size, (gc.B, gc.S), generator=g)
    hr.selfspec_batch(eng, ids, gc.GAMMA, gc.MAX_LEN, gc.EOT_1, gc.EOT_2, False)
    e = LMBackend(dtype=torch.bfloat16, device=DEV, dec_len=gc.GAMMA + 1, draft_dec_len=1)
    e.load_model(ck, use_tp=False)
    e.setup_caches(max_batch_size=gc.B, max_seq_length=gc.MAX_LEN, draft_budget=gc.BUDGET)
    st = replay(log, {"T": e}, {"T": _alt("snapkv_self", cfg, sd, gc.B, gc.MAX_LEN, gc.BUDGET)})
    parity_report(st.line(f"selfspec-snapkv/{name}"))


def test_cfg4_layout_lockstep_70b_target_with_different_streaming_draft():
    """BASELINE.json configs[3] in miniature on the GPU: a Llama-3.1-70B-like target (g = 8 -> two MFMA M tiles in the
    verify kernel) with a DIFFERENT, smaller StreamingLLM draft model (the layout of the reference-generated fixture
    run_longspec_stream_70b, tests/StreamingLLM/longspec_benchmark.py:241-278): the draft disagrees with the target
    on most steps, so the rejection / rollback paths run on every iteration (the all-accept two-token step is
    covered by the same-model longspec tests above)."""
    from magicdec_amd.Engine import model_core
    from magicdec_amd.Engine.SnapKV.backend import LMBackend
    from magicdec_amd.Engine.StreamingLLM.backend_draft import LMBackend_Draft
    cfg_t, sd_t, ck_t = _extra_ckpt("tiny70b")
    cfg_d, sd_d = gc.tiny("tinydrf")
    d = tempfile.mkdtemp(prefix="md_ckpt_")
    os.makedirs(os.path.join(d, "tinydrf"))
    torch.save(sd_d, os.path.join(d, "tinydrf", "model.pth"))
    model_core.transformer_configs["tinydrf"] = gc.config_kwargs(cfg_d)
    log = []
    tgt = Recorder(mr.RefEngine("target", cfg_t, sd_t, gc.B, gc.MAX_LEN), "T", log)
    drf = Recorder(mr.RefEngine("stream_draft", cfg_d, sd_d, gc.B, 0, gc.BUDGET), "D", log)
    accepted = []
    for ids in gc.synthetic_batches()[:N_BATCH]:
        out = hr.longspec_batch(tgt, drf, ids, gc.GAMMA, gc.MAX_LEN, gc.EOT_1, gc.EOT_2)
        accepted.append(out)
    n_cu = sum(1 for r in log if r["cu"] is not None)
    e_t = LMBackend(dtype=torch.bfloat16, device=DEV, dec_len=gc.GAMMA + 1)
    e_t.load_model(ck_t, use_tp=False)
    e_t.setup_caches(max_batch_size=gc.B, max_seq_length=gc.MAX_LEN)
    from pathlib import Path
    e_d = LMBackend_Draft(dtype=torch.bfloat16, device=DEV)
    e_d.load_model(Path(d) / "tinydrf" / "model.pth", use_tp=False)
    e_d.setup_caches(max_batch_size=gc.B, draft_budget=gc.BUDGET)
    alt = {"T": _alt("target", cfg_t, sd_t, gc.B, gc.MAX_LEN), "D": _alt("stream_draft", cfg_d, sd_d, gc.B, 0, gc.BUDGET)}
    st = replay(log, {"T": e_t, "D": e_d}, alt)
    n_verify = sum(1 for r in log if r["tag"] == "T" and r["fn"] == "inference")
    parity_report(st.line("cfg4: 70B-like + other stream draft") + f"  verify calls={n_verify} two-token draft steps={n_cu}")
    assert n_verify >= 20


def test_cfg5_layout_lockstep_qwen_selfspec_snapkv_fp8_cache():
    """BASELINE.json configs[4] in miniature on the GPU: Qwen2.5-like model (qkv bias, g = 5 -> padded second M tile,
    eps 1e-6) self-speculating over a SnapKV draft cache with the full-context cache stored as fp8 (e4m3fn).  The
    oracle is mr.RefEngine(kv_fp8=True): the same state machine over the EXACTLY dequantised cache (byte * scale in
    float32), quantising every appended row with the specification quantiser; the HIP engine is given the oracle's
    static scales (kv_scale_override) so that both quantise identically.  Same measured gates as the bf16 engines."""
    from magicdec_amd.Engine.SnapKV.backend import LMBackend
    cfg, sd, ck = _extra_ckpt("tinyqwen")
    log = []
    eng = Recorder(mr.RefEngine("snapkv_self", cfg, sd, gc.B, gc.MAX_LEN, gc.BUDGET, kv_fp8=True), "T", log)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(4, cfg.vocab_size, (gc.B, gc.S), generator=g)
    hr.selfspec_batch(eng, ids, gc.GAMMA, gc.MAX_LEN, gc.EOT_1, gc.EOT_2, False)
    e = LMBackend(dtype=torch.bfloat16, device=DEV, dec_len=gc.GAMMA + 1, draft_dec_len=1)
    e.load_model(ck, use_tp=False)
    e.setup_caches(max_batch_size=gc.B, max_seq_length=gc.MAX_LEN, draft_budget=gc.BUDGET, kv_dtype="fp8")
    st = replay(log, {"T": e}, {"T": _alt("snapkv_self", cfg, sd, gc.B, gc.MAX_LEN, gc.BUDGET, kv_fp8=True)})
    # the HIP cache bytes dequantise to the oracle's float32 cache wherever the appended k/v agreed bit for bit;
    # report how many bytes differ (1-ulp bf16 differences of k/v can move an fp8 rounding)
    kc = e.model.layers[0].attention.kv_cache
    hip = kc.kv_cache.float().cpu()
    if kc.layout == "HND":                     # MAGICDEC_KV_LAYOUT=HND: back to [pages, 2, 128, KH, D]
        hip = hip.permute(0, 1, 3, 2, 4).contiguous()
    hip[:, 0] *= kc.k_scale.cpu().view(1, 1, -1, 1)
    hip[:, 1] *= kc.v_scale.cpu().view(1, 1, -1, 1)
    ref = eng.eng.caches[0]
    frac = (hip != ref).float().mean().item()
    parity_report(st.line("cfg5: qwen-like g=5 selfspec, fp8 KV") + f"  layer-0 cache elements != oracle: {100 * frac:.3f}%")
    assert frac <= 0.02


def test_lockstep_with_every_linear_on_the_skinny_gemm(ckpt_dir):
    """MAGICDEC_GEMM=hip: every linear of the decode / verify steps (wqkv, wo, w1|w3 + fused SiLU*mul, w2, lm head)
    runs on md_linear over the streaming weight layout instead of hipBLASLt; same lock-step gates as the default
    policy (the tiny models are below the policy's size threshold, so this is the engine-level test of the kernel)."""
    from magicdec_amd.Engine import gemm_policy
    cfg, sd = gc.tiny("tinytgt")
    log = []
    tgt = Recorder(mr.RefEngine("target", cfg, sd, gc.B, gc.MAX_LEN), "T", log)
    drf = Recorder(mr.RefEngine("snapkv_draft", cfg, sd, gc.B, gc.MAX_LEN, gc.BUDGET), "D", log)
    hr.longspec_batch(tgt, drf, gc.synthetic_batches()[0], gc.GAMMA, gc.MAX_LEN, gc.EOT_1, gc.EOT_2)
    old = gemm_policy.mode()
    gemm_policy.set_mode("hip")
    try:
        e_t, e_d = _hip("target", ckpt_dir), _hip("snapkv_draft", ckpt_dir)
        assert len(e_t.model._packed) == 4 * cfg.n_layer + 1, "every weight should have a streaming-layout copy"
        st = replay(log, {"T": e_t, "D": e_d}, {"T": _alt("target", cfg, sd, gc.B, gc.MAX_LEN),
                                                 "D": _alt("snapkv_draft", cfg, sd, gc.B, gc.MAX_LEN, gc.BUDGET)})
    finally:
        gemm_policy.set_mode(old)
    parity_report(st.line("longspec/snapkv, all linears md_linear"))


def test_lockstep_with_every_linear_on_the_block_gemm(ckpt_dir):
    """MAGICDEC_BLOCK=1: every linear of the decode / verify steps of the tiny target (all N % 128 == 0, K % 64 == 0)
    runs on md_linear_block -- plain (wqkv, lm head), SwiGLU in the kernel / in the combine launch (w1|w3) and the
    residual add + RMSNorm combine (wo, w2) -- under the same lock-step gates as the default policy (the BASELINE shapes
    that take this kernel by the measured rule, N >= 20480, do not occur in the tiny models)."""
    from magicdec_amd.Engine import gemm_policy
    cfg, sd = gc.tiny("tinytgt")
    log = []
    tgt = Recorder(mr.RefEngine("target", cfg, sd, gc.B, gc.MAX_LEN), "T", log)
    drf = Recorder(mr.RefEngine("snapkv_draft", cfg, sd, gc.B, gc.MAX_LEN, gc.BUDGET), "D", log)
    hr.longspec_batch(tgt, drf, gc.synthetic_batches()[0], gc.GAMMA, gc.MAX_LEN, gc.EOT_1, gc.EOT_2)
    old = gemm_policy.block_mode()
    gemm_policy.set_block("1")
    try:
        assert gemm_policy.choose(8, 768, 512, False, False, True, "qkv") == "block"
        e_t, e_d = _hip("target", ckpt_dir), _hip("snapkv_draft", ckpt_dir)
        assert len(e_t.model._packed) == 4 * cfg.n_layer + 1
        st = replay(log, {"T": e_t, "D": e_d}, {"T": _alt("target", cfg, sd, gc.B, gc.MAX_LEN),
                                                 "D": _alt("snapkv_draft", cfg, sd, gc.B, gc.MAX_LEN, gc.BUDGET)})
    finally:
        gemm_policy.set_block(old)
    parity_report(st.line("longspec/snapkv, all linears md_linear_block"))


def test_int8_weight_only_engine_lockstep():
    """Weight-only int8 (Engine/quantize.py, "int8" in the checkpoint path -> Engine/utils.py:201-205): the tiny
    target quantised per channel, loaded through the int8 loader, every linear streamed as int8 by md_linear with the
    fused bf16 scale epilogue; lock-step against the oracle running F.linear(x, w.to(bf16)) * scales."""
    from pathlib import Path
    from magicdec_amd.Engine import model_core
    from magicdec_amd.Engine.quantize import WeightOnlyInt8Linear, dynamically_quantize_per_channel
    from magicdec_amd.Engine.SnapKV.backend import LMBackend
    cfg, sd = gc.tiny("tinytgt")
    qsd = {}
    for k, v in sd.items():
        if k.endswith(".weight") and v.dim() == 2 and "tok_embeddings" not in k:
            q, sc, _ = dynamically_quantize_per_channel(v.float(), -128, 127, torch.int8)
            qsd[k], qsd[k[:-len("weight")] + "scales"] = q, sc.to(torch.bfloat16)
        else:
            qsd[k] = v
    d = tempfile.mkdtemp(prefix="md_ckpt_")
    os.makedirs(os.path.join(d, "tinytgt-int8"))
    torch.save(qsd, os.path.join(d, "tinytgt-int8", "model.pth"))
    model_core.transformer_configs["tinytgt"] = gc.config_kwargs(cfg)
    log = []
    eng = Recorder(mr.RefEngine("target", cfg, qsd, gc.B, gc.MAX_LEN), "T", log)
    hr.baseline_batch(eng, gc.synthetic_batches()[0], gc.S + 24, -1, -1)
    e = LMBackend(dtype=torch.bfloat16, device=DEV)
    e.load_model(Path(d) / "tinytgt-int8" / "model.pth", use_tp=False)
    e.setup_caches(max_batch_size=gc.B, max_seq_length=gc.MAX_LEN)
    assert isinstance(e.model.layers[0].attention.wqkv, WeightOnlyInt8Linear)
    assert e.model.layers[0].feed_forward.w2.weight.dtype == torch.int8
    st = replay(log, {"T": e}, {"T": _alt("target", cfg, qsd, gc.B, gc.MAX_LEN)})
    parity_report(st.line("baseline, weight-only int8 linears"))


def test_baseline_llama68m_shape_lockstep():
    """BASELINE.json configs[0]: llama-68m autoregressive baseline, B=1, prefix 129 (MHA, D=64, vocab 32000)."""
    from magicdec_amd.Engine.SnapKV.backend import LMBackend
    cfg, sd, ck = _extra_ckpt("tiny68m")
    log = []
    eng = Recorder(mr.RefEngine("target", cfg, sd, 1, 256), "T", log)
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(4, cfg.vocab_size, (1, 129), generator=g)
    out = hr.baseline_batch(eng, ids, 256, -1, -1)
    assert out["steps"] == 126 and eng.cachelens.tolist() == [255] and eng.paged_kv_last_page_len.tolist() == [127]
    e = LMBackend(dtype=torch.bfloat16, device=DEV)
    e.load_model(ck, use_tp=False)
    e.setup_caches(max_batch_size=1, max_seq_length=256)
    st = replay(log, {"T": e}, {"T": _alt("target", cfg, sd, 1, 256)})
    parity_report(st.line("baseline/68m-like"))


def test_tp2_on_one_gpu(ckpt_dir, graphs=False):
    """Tensor parallel degree 2 with the HIP kernels on KV-head shards (both ranks on the box's single GPU) and the
    one-shot IPC all-reduce: the two ranks end with bit-identical replicated state (outputs, lengths), no peer
    time-outs, and the teacher-forced TP=2 logits (vocab shards concatenated) equal the TP=1 HIP engine's within
    4 bf16 ulps at the logit scale (the partial sums are rounded to bf16 before the all-reduce: a rounding point TP=1
    does not have).
    Eager steps only: in this one-GPU configuration the bootstrap transport is gloo, whose argmax-merge all-reduce
    stages through the host and cannot be captured; the one-shot kernel under hipGraph replay is covered by
    tests/test_gpu_allreduce.py and RCCL-in-graph by profiles/r01_tp1rank_rccl_graphs.log."""
    import json
    import subprocess
    import sys
    from magicdec_amd import harness
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tempfile.mkdtemp(prefix="md_tp_gpu_")
    port = 29700 + (os.getpid() % 200) + (1 if graphs else 0)
    procs = []
    for r in range(2):
        env = dict(os.environ, LOCAL_RANK=str(r), LOCAL_WORLD_SIZE="2", RANK=str(r), WORLD_SIZE="2",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), MD_CKPT=str(ckpt_dir), MD_OUT=out,
                   MAGICDEC_TP_SINGLE_GPU="1", MAGICDEC_ONESHOT_AR="1", HSA_ENABLE_IPC_MODE_LEGACY="0",
                   MD_GRAPHS="1" if graphs else "0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "tests", "_tp_gpu_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=400)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    r0, r1 = (json.load(open(os.path.join(out, f"rank{r}.json"))) for r in range(2))
    assert r0["local_heads"] == [4, 1] and r1["local_heads"] == [4, 1]
    assert r0["output"] == r1["output"] and r0["num_nodes"] == r1["num_nodes"] and r0["cachelens"] == r1["cachelens"]
    assert r0["iters"] == r1["iters"] and r0["iters"] > 3
    assert r0["ar_status"] == [0, 0] and r1["ar_status"] == [0, 0]
    probe = r0["collectives"]["probe"]
    assert probe["xgmi_timeouts"] == 0 and all(probe[k] > 0 for k in ("rccl_allreduce", "xgmi_oneshot", "xgmi_twoshot",
                                                                      "xgmi_fused_add_rmsnorm_auto")), probe
    # the bit-exact stress bench.py's N > 1 runs select the collective by: 640 queued calls, every element equal to "sum
    # in rank order, fp32, one rounding"
    stress = r0["collectives"]["xgmi_stress"]
    assert stress["calls"] >= 600 and stress["mismatched_elements_all_ranks"] == 0 and stress["timeouts_all_ranks"] == 0, stress
    # numerics of the sharded engine: teacher-forced logits (vocab shards concatenated) vs the TP=1 HIP engine
    tgt, drf = _hip("target", ckpt_dir), _hip("snapkv_draft", ckpt_dir)
    ids = gc.synthetic_batches()[0].to(DEV)
    tgt.encode(ids)
    tgt.inference(ids[:, :gc.GAMMA + 1].clone())
    l1 = tgt.model._last_logits.float().cpu()
    l2 = torch.cat([torch.load(os.path.join(out, f"logits_rank{r}.pt")) for r in range(2)], dim=1)
    err = (l1 - l2).abs().max().item()
    ulp = _ulp_at(l1.abs().max().item())
    parity_report(f"[TP2 vs TP1] max |logit diff| = {err:.4f} = {err / ulp:.2f} bf16 ulp "
                  f"(logit range {l1.min().item():.2f}..{l1.max().item():.2f})")
    assert l1.shape == l2.shape and err <= 4 * ulp      # partials are rounded to bf16 before the all-reduce
    st, _ = harness.run_longspec_batch(tgt, drf, ids, gc.GAMMA, gc.MAX_LEN, gc.EOT_1, gc.EOT_2)
    one = st.output.cpu()
    two = torch.tensor(r0["output"])
    agree = total = 0
    for b in range(gc.B):
        n = min(int(st.num_nodes[b]), int(r0["num_nodes"][b]))
        a, c = one[b, gc.S:n], two[b, gc.S:n]
        neq = torch.nonzero(a != c)
        agree += int(neq[0]) if len(neq) else len(a)
        total += len(a)
    # free-running greedy sequences of a random tiny model diverge at the first near-tie and never re-join, so the
    # agreeing prefix is reported, not gated (the logits above are the gate)
    parity_report(f"[TP2 vs TP1] free-running agreeing prefix {agree}/{total} generated tokens")
    assert total > 0


def test_bench_tp_code_path_with_rccl_graphs_one_rank():
    """bench.py on the tensor-parallel code path (RCCL process group of one rank, models sharded as rank 0 of 2,
    per-layer all-reduces and the TP argmax merge captured inside the hipGraph steps): runs to completion, the JSON
    line is the LAST line of stdout (RCCL's stdio banner must not trail it) and the steps really were graphs.
    Guards two multi-GPU-only failures found this round: the RCCL watchdog's event queries killing a global-mode
    capture, and the buffered RCCL banner landing after the JSON line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29800 + os.getpid() % 100))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "tiny", "--emulate-tp", "2",
                        "--no-cpu-baseline", "--steps", "8", "--warmup", "2", "--full"], env=env, cwd=root,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    last = [l for l in p.stdout.splitlines() if l.strip()][-1]
    line = json.loads(last)
    assert line["config"]["hip_graphs"] is True and line["config"]["allreduce"] == "rccl"
    assert line["config"]["emulated_tp_rank0_of"] == 2 and line["value"] > 0 and line["roofline"]["traffic"] is None


def test_longspec_full_kv_draft_lockstep_with_oracle(ckpt_dir):
    """--draft_budget -1 (the reference script's default): a different, smaller draft model decoding over its FULL KV
    cache (no SnapKV select, frequent rejections -> the rollback and two-token paths), replayed in lock-step against
    the oracle (which is pinned to the real reference's run of this layout: run_longspec_snapkv_fullkv)."""
    from pathlib import Path
    from magicdec_amd.Engine.SnapKV.backend_draft import LMBackend_Draft
    cfg_t, sd_t = gc.tiny("tinytgt")
    cfg_d, sd_d = gc.tiny("tinydrf")
    log = []
    tgt = Recorder(mr.RefEngine("target", cfg_t, sd_t, gc.B, gc.MAX_LEN), "T", log)
    drf = Recorder(mr.RefEngine("snapkv_draft", cfg_d, sd_d, gc.B, gc.MAX_LEN, -1), "D", log)
    for ids in gc.synthetic_batches()[:1]:
        hr.longspec_batch(tgt, drf, ids, gc.GAMMA, gc.MAX_LEN, gc.EOT_1, gc.EOT_2)
    e_d = LMBackend_Draft(dtype=torch.bfloat16, device=DEV, draft_budget=-1)
    e_d.load_model(Path(ckpt_dir) / "tinydrf" / "model.pth", use_tp=False)
    e_d.setup_caches(max_batch_size=gc.B, max_seq_length=gc.MAX_LEN, draft_budget=-1)
    alt = {"T": _alt("target", cfg_t, sd_t, gc.B, gc.MAX_LEN), "D": _alt("snapkv_draft", cfg_d, sd_d, gc.B, gc.MAX_LEN, -1)}
    st = replay(log, {"T": _hip("target", ckpt_dir), "D": e_d}, alt)
    n_cu = sum(1 for r in log if r["cu"] is not None)
    parity_report(st.line("longspec, full-KV draft (budget -1)") + f"  two-token draft steps={n_cu}")


def test_batch_size_one_selfspec_stream_lockstep_with_oracle(ckpt_dir):
    """B = 1 (the reference scripts' default batch size): StreamingLLM self-speculation with one request -- one-block
    grids in every kernel -- in lock-step against the oracle (pinned to the reference's B = 1 run:
    run_selfspec_stream_b1)."""
    from pathlib import Path
    from magicdec_amd.Engine.StreamingLLM.backend import LMBackend
    cfg, sd = gc.tiny("tinytgt")
    log = []
    eng = Recorder(mr.RefEngine("stream_self", cfg, sd, 1, gc.MAX_LEN, gc.BUDGET), "T", log)
    g = torch.Generator().manual_seed(123)
    ids = torch.randint(4, cfg.vocab_size, (1, gc.S), generator=g)
    ids[:, 0] = 1
    hr.selfspec_batch(eng, ids, gc.GAMMA, gc.MAX_LEN, gc.EOT_1, gc.EOT_2, True)
    e = LMBackend(dtype=torch.bfloat16, device=DEV, dec_len=gc.GAMMA + 1)
    e.load_model(Path(ckpt_dir) / "tinytgt" / "model.pth", use_tp=False)
    e.setup_caches(max_batch_size=1, max_seq_length=gc.MAX_LEN, draft_budget=gc.BUDGET)
    st = replay(log, {"T": e}, {"T": _alt("stream_self", cfg, sd, 1, gc.MAX_LEN, gc.BUDGET)})
    parity_report(st.line("selfspec/stream_self, B = 1"))


def test_selfspec_snapkv_lockstep_with_a_prefix_of_several_score_chunks(ckpt_dir):
    """The same lock-step with a 1184-token prompt (10 prefill chunks; 1152 candidate columns = two of the SnapKV
    kernel's 1024-column score chunks inside the engine flow; verify over 10 pages) instead of the 416 of the other
    engine tests."""
    from pathlib import Path
    from magicdec_amd.Engine.SnapKV.backend import LMBackend
    S, ML = 1184, 1280
    cfg, sd = gc.tiny("tinytgt")
    log = []
    eng = Recorder(mr.RefEngine("snapkv_self", cfg, sd, gc.B, ML, gc.BUDGET), "T", log)
    g = torch.Generator().manual_seed(77)
    ids = torch.randint(4, cfg.vocab_size, (gc.B, S), generator=g)
    ids[:, 0] = 1
    hr.selfspec_batch(eng, ids, gc.GAMMA, ML, gc.EOT_1, gc.EOT_2, False)
    e = LMBackend(dtype=torch.bfloat16, device=DEV, dec_len=gc.GAMMA + 1, draft_dec_len=1)
    e.load_model(Path(ckpt_dir) / "tinytgt" / "model.pth", use_tp=False)
    e.setup_caches(max_batch_size=gc.B, max_seq_length=ML, draft_budget=gc.BUDGET)
    st = replay(log, {"T": e}, {"T": _alt("snapkv_self", cfg, sd, gc.B, ML, gc.BUDGET)})
    parity_report(st.line("selfspec/snapkv_self, prefix 1184"))


def test_selfspec_stream_lockstep_at_the_baseline_budget_257(ckpt_dir):
    """BASELINE configs[1]'s draft geometry: StreamingLLM self-speculation with budget 257 (3 draft pages per request:
    the eviction shifts rows across page boundaries at every prefill chunk) and a 1184-token prompt."""
    from pathlib import Path
    from magicdec_amd.Engine.StreamingLLM.backend import LMBackend
    S, ML, budget = 1184, 1280, 257
    cfg, sd = gc.tiny("tinytgt")
    log = []
    eng = Recorder(mr.RefEngine("stream_self", cfg, sd, gc.B, ML, budget), "T", log)
    g = torch.Generator().manual_seed(78)
    ids = torch.randint(4, cfg.vocab_size, (gc.B, S), generator=g)
    ids[:, 0] = 1
    hr.selfspec_batch(eng, ids, gc.GAMMA, ML, gc.EOT_1, gc.EOT_2, True)
    e = LMBackend(dtype=torch.bfloat16, device=DEV, dec_len=gc.GAMMA + 1)
    e.load_model(Path(ckpt_dir) / "tinytgt" / "model.pth", use_tp=False)
    e.setup_caches(max_batch_size=gc.B, max_seq_length=ML, draft_budget=budget)
    st = replay(log, {"T": e}, {"T": _alt("stream_self", cfg, sd, gc.B, ML, budget)})
    parity_report(st.line("selfspec/stream_self, budget 257, prefix 1184"))


def _peaked_wide(cfg, seed, emb_rms=40.0, peak=12.0, miss_every=0):
    """Seeded weights of `cfg` with peaked next-token distributions (the construction of golden_cfg.peaked_pair /
    Engine/utils._peak_ at any width): dominant embedding, head tied to it through a permutation that depends on the
    vocabulary only -- two models of one vocabulary predict through the same map, except that a model built with
    `miss_every` = m mispredicts every m-th token id (a draft that is rejected at a known rate)."""
    sd = mr.init_state_dict(cfg, seed)
    g = torch.Generator().manual_seed(4242 + cfg.vocab_size)
    perm = torch.arange(cfg.vocab_size)
    perm[4:] = 4 + torch.randperm(cfg.vocab_size - 4, generator=g)
    if miss_every:
        miss = torch.arange(4, cfg.vocab_size, miss_every)
        perm = perm.clone()
        perm[miss] = perm[torch.roll(miss, 1)]
    e = sd["tok_embeddings.weight"].float() * (emb_rms / 0.02)
    sd["tok_embeddings.weight"] = e.to(torch.bfloat16)
    sd["output.weight"] = (e[perm] * (peak / (cfg.dim * emb_rms))).to(torch.bfloat16)
    return sd


def test_full_width_8b_and_1b_layers_b64_lockstep_token_identity():
    """every other engine-level test runs models of dim <= 2048 at B <= 4, i.e. none of the kernels
    the BASELINE configuration selects.  Here the layers have the REAL widths of configs[2] -- target: Llama-3.1-8B
    (dim 4096, 32 / 8 heads, D = 128, FFN 14336, vocab 128 256, llama-3.1 RoPE), draft: Llama-3.2-1B (dim 2048, D = 64,
    FFN 8192) with a SnapKV cache (budget 129) -- at the REAL batch (B = 64: 256-row verify -> md_linear_block, the
    M = 256 library products, the two-M-tile-free 16-row MFMA attention; 64-row draft steps -> md_linear_fused /
    md_linear; the 128 256-column head and argmax), only with 2 layers each and a 160-token prompt so that the CPU
    oracle finishes in about a minute.  The weights are peaked (the oracle's top-2 gap is asserted), so the HIP engines
    must reproduce EVERY token of EVERY call of the oracle's longspec run (the draft mispredicts a quarter of the token
    ids: rejections, rollbacks, bonus tokens and the two-token draft step after an all-accept iteration are in the run),
    the integer state exactly, and the logits within 4 bf16 ulps of the largest logit (no float64 yardsticks at this width: a float64 128 256-row head costs
    seconds per call)."""
    from pathlib import Path
    from magicdec_amd.Engine import model_core
    from magicdec_amd.Engine.SnapKV.backend import LMBackend
    from magicdec_amd.Engine.SnapKV.backend_draft import LMBackend_Draft
    l31 = dict(rope_base=500000.0, scaling_factor=8, high_freq_factor=4, low_freq_factor=1,
               original_max_position_embeddings=8192)
    cfg_t = mr.RefConfig(n_layer=2, n_head=32, n_local_heads=8, dim=4096, intermediate_size=14336, vocab_size=128256, **l31)
    cfg_d = mr.RefConfig(n_layer=2, n_head=32, n_local_heads=8, dim=2048, intermediate_size=8192, vocab_size=128256,
                         **dict(l31, scaling_factor=32))
    B, S, ML, G, BUD = 64, 160, 256, 3, 129
    with capped_threads():
        sd_t, sd_d = _peaked_wide(cfg_t, 31), _peaked_wide(cfg_d, 32, miss_every=4)     # a quarter of the drafts rejected
    d = tempfile.mkdtemp(prefix="md_wide_")
    for name, cfg, sd in (("wide8b", cfg_t, sd_t), ("wide1b", cfg_d, sd_d)):
        os.makedirs(os.path.join(d, name))
        torch.save(sd, os.path.join(d, name, "model.pth"))
        model_core.transformer_configs[name] = gc.config_kwargs(cfg)
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(4, cfg_t.vocab_size, (B, S), generator=g)
    ids[:, 0] = 1
    log = []
    tgt = Recorder(mr.RefEngine("target", cfg_t, sd_t, B, ML), "T", log)
    drf = Recorder(mr.RefEngine("snapkv_draft", cfg_d, sd_d, B, ML, BUD), "D", log)
    with capped_threads():
        iters = hr.longspec_batch(tgt, drf, ids, G, ML, -1, -2)["iters"]
    npos = wide = 0
    for rec in log:
        lg = rec["logits"].view(-1, rec["logits"].shape[-1])
        top2 = lg.topk(2, dim=-1).values
        ulp = torch.tensor([_ulp_at(float(v)) for v in top2[:, 0]])
        npos += lg.shape[0]
        wide += int(((top2[:, 0] - top2[:, 1]) >= 16 * ulp).sum())
    assert wide >= 0.99 * npos, (npos, wide)
    import shutil
    try:
        e_t = LMBackend(dtype=torch.bfloat16, device=DEV, dec_len=G + 1)
        e_t.load_model(Path(d) / "wide8b" / "model.pth", use_tp=False)
        e_t.setup_caches(max_batch_size=B, max_seq_length=ML)
        e_d = LMBackend_Draft(dtype=torch.bfloat16, device=DEV, draft_budget=BUD)
        e_d.load_model(Path(d) / "wide1b" / "model.pth", use_tp=False)
        e_d.setup_caches(max_batch_size=B, max_seq_length=ML, draft_budget=BUD)
    finally:
        shutil.rmtree(d, ignore_errors=True)          # 3 GB of checkpoints: gone whether or not the load worked
        for name in ("wide8b", "wide1b"):             # the config table is process-global
            model_core.transformer_configs.pop(name, None)
    st = replay(log, {"T": e_t, "D": e_d}, None)
    verify_rows = sum(r["out"].numel() for r in log if r["tag"] == "T" and r["fn"] == "inference")
    n_two = sum(1 for r in log if r["cu"] is not None)
    assert n_two >= 1, "no two-token draft step in the run"
    parity_report(f"[lockstep] full-width 8B + 1B layers, B = 64 (2 layers each) calls={st.calls:4d} positions={st.npos:6d} "
                  f"argmax flips vs the oracle: hip={st.nties:3d}  max|hip-oracle|={st.err_hip:.4f}  worst err_hip / "
                  f"(4 ulp)={st.worst_ratio:.3f}  | top-2 gap >= 16 ulp on {wide}/{npos} positions, {iters} iterations, "
                  f"{verify_rows} verify positions, {n_two} two-token draft steps")
    assert st.nties == 0, f"{st.nties} tokens differ from the oracle's at full width"
    assert iters >= 10 and st.npos >= 10000


def _deep(cfg, sd, n_layer):
    """`sd` (weights of a `cfg.n_layer`-layer model) stretched to `n_layer` layers by CYCLING its layers (layer i takes the
    tensors of layer i % cfg.n_layer: aliases, no copies) -- 32 + 16 layers of distinct seeded tensors would take minutes
    of single-threaded randn and 19 GB of host memory before the test starts; what is under test, the rounding a real
    depth of real-width layers accumulates, does not depend on the layers being pairwise different."""
    import dataclasses
    out = {k: v for k, v in sd.items() if not k.startswith("layers.")}
    for i in range(n_layer):
        src = f"layers.{i % cfg.n_layer}."
        for k, v in sd.items():
            if k.startswith(src):
                out[f"layers.{i}." + k[len(src):]] = v
    return dataclasses.replace(cfg, n_layer=n_layer), out


def test_full_depth_8b_and_1b_lockstep_token_identity(monkeypatch):
    """VERDICT r5 missing #5 / next #5: nothing compared 32 layers of dim 4096 of accumulated bf16 rounding with the
    oracle -- the full-width lock-step above is 2 layers each.  Here the models have the REAL depth and width of
    configs[2]: target 32 layers x dim 4096 (32 / 8 heads, D = 128, FFN 14336, vocab 128 256, llama-3.1 RoPE), draft
    16 layers x dim 2048 (D = 64, FFN 8192) with a SnapKV cache (budget 129); B = 2, prefix 160, gamma 3, the whole
    80-token generation of the reference's longspec loop (>= 5 iterations asserted; the draft mispredicts a quarter of
    the token ids, so rejections, rollbacks and bonus tokens are in the run).  Peaked weights (Engine/utils._peak_'s
    construction; the oracle's top-2 gap is asserted), four distinct seeded layers cycled to the full depth (_deep).
    Bar: EVERY token of EVERY call equals the oracle's (0 flips), the integer state exactly, the logits within 4 bf16
    ulps of the largest logit -- after 32 (16) layers, the final norm and the 128 256-row head."""
    from pathlib import Path
    from magicdec_amd.Engine import model_core, utils
    from magicdec_amd.Engine.SnapKV.backend import LMBackend
    from magicdec_amd.Engine.SnapKV.backend_draft import LMBackend_Draft
    l31 = dict(rope_base=500000.0, scaling_factor=8, high_freq_factor=4, low_freq_factor=1,
               original_max_position_embeddings=8192)
    c4_t = mr.RefConfig(n_layer=4, n_head=32, n_local_heads=8, dim=4096, intermediate_size=14336, vocab_size=128256, **l31)
    c4_d = mr.RefConfig(n_layer=4, n_head=32, n_local_heads=8, dim=2048, intermediate_size=8192, vocab_size=128256,
                        **dict(l31, scaling_factor=32))
    B, S, ML, G, BUD = 2, 160, 256, 3, 129
    with capped_threads():
        cfg_t, sd_t = _deep(c4_t, _peaked_wide(c4_t, 41), 32)
        cfg_d, sd_d = _deep(c4_d, _peaked_wide(c4_d, 42, miss_every=4), 16)
    g = torch.Generator().manual_seed(19)
    ids = torch.randint(4, cfg_t.vocab_size, (B, S), generator=g)
    ids[:, 0] = 1
    log = []
    tgt = Recorder(mr.RefEngine("target", cfg_t, sd_t, B, ML), "T", log)
    drf = Recorder(mr.RefEngine("snapkv_draft", cfg_d, sd_d, B, ML, BUD), "D", log)
    with capped_threads():
        iters = hr.longspec_batch(tgt, drf, ids, G, ML, -1, -2)["iters"]
    npos = wide = 0
    for rec in log:
        lg = rec["logits"].view(-1, rec["logits"].shape[-1])
        top2 = lg.topk(2, dim=-1).values
        ulp = torch.tensor([_ulp_at(float(v)) for v in top2[:, 0]])
        npos += lg.shape[0]
        wide += int(((top2[:, 0] - top2[:, 1]) >= 16 * ulp).sum())
    assert wide >= 0.99 * npos, (npos, wide)
    # the HIP engines load the SAME tensors: a checkpoint file of 16 + 2.5 GB is not written -- torch.load is answered from
    # memory for the two placeholder paths (Engine/utils._load only asks whether the file exists, then loads it)
    d = tempfile.mkdtemp(prefix="md_deep_")
    sds = {}
    for name, cfg, sd in (("deep8b", cfg_t, sd_t), ("deep1b", cfg_d, sd_d)):
        os.makedirs(os.path.join(d, name))
        Path(d, name, "model.pth").write_bytes(b"")
        sds[str(Path(d, name, "model.pth"))] = sd
        model_core.transformer_configs[name] = gc.config_kwargs(cfg)
    real_load = torch.load
    monkeypatch.setattr(utils.torch, "load", lambda f, *a, **k: dict(sds[str(f)]) if str(f) in sds else real_load(f, *a, **k))
    import shutil
    try:
        e_t = LMBackend(dtype=torch.bfloat16, device=DEV, dec_len=G + 1)
        e_t.load_model(Path(d) / "deep8b" / "model.pth", use_tp=False)
        e_t.setup_caches(max_batch_size=B, max_seq_length=ML)
        e_d = LMBackend_Draft(dtype=torch.bfloat16, device=DEV, draft_budget=BUD)
        e_d.load_model(Path(d) / "deep1b" / "model.pth", use_tp=False)
        e_d.setup_caches(max_batch_size=B, max_seq_length=ML, draft_budget=BUD)
    finally:
        shutil.rmtree(d, ignore_errors=True)
        for name in ("deep8b", "deep1b"):             # the config table is process-global
            model_core.transformer_configs.pop(name, None)
    assert len(e_t.model.layers) == 32 and len(e_d.model.layers) == 16
    st = replay(log, {"T": e_t, "D": e_d}, None)
    verify_rows = sum(r["out"].numel() for r in log if r["tag"] == "T" and r["fn"] == "inference")
    rejected = sum(int((r["post"]["cachelens"] - r["pre"]["cachelens"]).sum()) for r in log
                   if r["tag"] == "T" and r["fn"] == "inference")
    parity_report(f"[lockstep] FULL DEPTH 8B (32 x dim 4096) + 1B (16 x dim 2048), B = {B}, prefix {S} calls={st.calls:4d} "
                  f"positions={st.npos:6d} argmax flips vs the oracle: hip={st.nties:3d}  max|hip-oracle|={st.err_hip:.4f}  "
                  f"worst err_hip / (4 ulp)={st.worst_ratio:.3f}  | top-2 gap >= 16 ulp on {wide}/{npos} positions, "
                  f"{iters} iterations, {verify_rows} verify positions")
    assert st.nties == 0, f"{st.nties} tokens differ from the oracle's at full depth"
    assert iters >= 5 and rejected >= 0
    del e_t, e_d
    torch.cuda.empty_cache()


def test_rowmajor_weights_are_released_after_prefill_and_restored_for_the_next(ckpt_dir):
    """Round 6: after encode() the row-major tensor of every weight that the decode steps of THIS
    engine read in the streaming layout only is released (Transformer.release_rowmajor) -- one resident copy; the next
    encode() re-materialises them from the streaming copy.  On the HIP engine: bytes are really released, decode and
    verify steps run on the released state, and a second encode + decode reproduces the first run's tokens and logits bit
    for bit (the restored tensors are the originals)."""
    e = _hip("target", ckpt_dir)
    m = e.model
    ids = gc.synthetic_batches()[0].to(DEV)
    assert m.decode_rows == tuple(sorted({gc.B, gc.B * (gc.GAMMA + 1)}))        # a longspec target: no two-token step
    total = sum(p.data.numel() * p.data.element_size() for p in m._packed.values())
    assert total > 0 and m.packed_bytes == total and m.released_bytes == 0           # before the first prefill: both layouts
    t1 = e.encode(ids).clone()
    assert m.released_bytes > 0 and m.packed_bytes == total - m.released_bytes       # released at the end of encode()
    released = set(m._released)
    for k in released:
        assert m._by_id[k].stride() == (0, 0)                                         # no storage behind the Parameter
    step = e.inference(t1[:, -1:].clone()).clone()
    lg_step = m._last_logits.clone()
    ver = e.inference(torch.cat([t1[:, -1:], step, step, step], dim=1)).clone()      # a (gamma+1)-row verify
    lg_ver = m._last_logits.clone()
    t2 = e.encode(ids).clone()                                                        # restore -> prefill -> release again
    assert set(m._released) == released
    assert torch.equal(t1, t2)
    assert torch.equal(e.inference(t2[:, -1:].clone()), step) and torch.equal(m._last_logits, lg_step)
    assert torch.equal(e.inference(torch.cat([t2[:, -1:], step, step, step], dim=1)), ver)
    assert torch.equal(m._last_logits, lg_ver)
    # a row count nobody announced still computes (library GEMM on a per-call unpacked weight), it is only slower
    odd = e.inference(torch.cat([t2[:, -1:], step, step], dim=1))
    assert odd.shape == (gc.B, 3)
    parity_report(f"[weights] one resident copy: {len(released)} of {len(m._packed)} packed weights released after prefill "
                  f"({m.released_bytes} B), {m.packed_bytes} B still held in both layouts; re-encode reproduces tokens and "
                  f"logits bit for bit")


@pytest.mark.parametrize("kind", ["python_error", "illegal_sync"])
def test_a_failed_graph_capture_falls_back_to_eager_and_keeps_working(kind):
    """Engine/graph.py: a decode step whose hipGraph capture fails -- (a) an exception raised by Python code inside the
    capture, (b) an operation that is illegal while capturing and INVALIDATES it (a device synchronisation: what a
    collective that cannot be captured does; found by a 2-rank bench rehearsal over gloo) -- must leave the back-end
    running eagerly with the right results.  In a child process (tests/_graph_failure_worker.py): an invalidated capture
    leaves this PyTorch build unable to capture again in the same process, which must not leak into the other tests."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "_graph_failure_worker.py"), kind],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-4000:]
    parity_report(f"[graphs] capture failure ({kind}): " + [l for l in p.stdout.splitlines() if l.startswith("OK")][0])
