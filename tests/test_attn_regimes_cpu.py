"""The score-regime generator (tests/attn_regimes.py) and the attention gate, without a GPU.

For every regime, head dim and sm_scale: (1) the achieved float64 score statistics lie inside the bands the regime
declares; (2) the fp32 oracle passes tests/parity_util.check_attention; (3) a plain-torch emulation of the kernels'
algorithm (fp32 scores, online softmax over 32-key tiles from m = -1e30, P rounded to bf16, fp32 accumulation; one
pass, and four KV splits merged with the merge kernel's formula) passes the same gate and reproduces the saturated rows
bit for bit.  This is the proof that a CORRECT implementation stays inside the unchanged gate on these inputs, and the
printed `max err/bound` figures are what the GPU ratios of tests/test_gpu_attn_regimes.py are read against.
"""
import pytest
import torch

from oracle import flashinfer_ref as fr
from tests import attn_regimes as ar
from tests.conftest import parity_report
from tests.parity_util import check_attention, dense_attention_f64

N, KH, G, LENS = 4, 2, 4, [1000, 333]


def _id(s):
    return "default" if s is None else str(s)


def _gate(tag, pt, D, sm, scales=None):
    H = KH * G
    args = (pt["q"], pt["ref_cache"], pt["qo"], pt["indices"], pt["indptr"], pt["last"], H, KH, D)
    oracle = fr.batch_prefill_paged(*args, causal=True, sm_scale=sm)
    ref64, bnd = dense_attention_f64(*args, causal=True, sm_scale=sm)
    worst = {"oracle": check_attention(f"cpu {tag} oracle", oracle, oracle, ref64, bnd)}
    outs = {}
    for ns in (1, 4):
        outs[ns] = ar.emulate_paged(pt, KH, sm, causal=True, nsplit=ns)
        worst[ns] = check_attention(f"cpu {tag} emulation x{ns}", outs[ns], oracle, ref64, bnd)
    return worst, outs


@pytest.mark.parametrize("sm_scale", ar.SM_SCALES, ids=_id)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("regime", ar.REGIMES)
def test_regime_statistics_and_gate(regime, D, sm_scale):
    sm = ar.default_scale(D) if sm_scale is None else sm_scale
    reqs = [ar.make_request(regime, N, L, KH, G, D, seed=3 + b, sm_scale=sm_scale) for b, L in enumerate(LENS)]
    st = ar.score_stats(reqs[0], sm)
    for key, (lo, hi) in reqs[0].bands.items():
        assert lo <= st[key] <= hi, f"{regime} D{D} sm_scale {sm}: {key} = {st[key]:.4g} outside [{lo:.4g}, {hi:.4g}]"
    pt = ar.build_paged(reqs, seed=D)
    worst, _ = _gate(f"{regime} D{D} sm {_id(sm_scale)}", pt, D, sm)
    parity_report(f"[attn-regime] {regime:10s} D{D:<3d} sm_scale {_id(sm_scale):7s} L={LENS[0]}: score std {st['std']:8.3f} nats, "
                  f"max |s| {st['max_abs']:8.2f}, span {st['span']:8.2f}, mean max-p {st['maxp']:.3f} | max err/bound: oracle "
                  f"{worst['oracle']:.3f}, emulation {worst[1]:.3f}, 4 splits {worst[4]:.3f}")


@pytest.mark.parametrize("sm_scale", ar.SM_SCALES, ids=_id)
@pytest.mark.parametrize("D,n,g,fp8,causal", [(64, 4, 4, False, True), (128, 4, 8, False, True), (128, 4, 5, True, True),
                                              (64, 1, 4, True, True), (128, 100, 4, False, True), (128, 4, 4, False, False)])
def test_saturated_rows_are_bit_exact_in_the_emulation(D, n, g, fp8, causal, sm_scale):
    sm = ar.default_scale(D) if sm_scale is None else sm_scale
    scales = ar.pow2_scales(KH, D + n) if fp8 else None
    reqs = [ar.saturated_request(n, L, KH, g, D, seed=5 + b, sm_scale=sm_scale, causal=causal,
                                 k_scale=scales[0] if fp8 else None) for b, L in enumerate([1100, 333])]
    gap = min(ar.saturated_gap_log2(r, sm, causal) for r in reqs)
    assert gap >= ar.SAT_GAP_LOG2
    pt = ar.build_paged(reqs, seed=n, scales=scales)
    if fp8:       # the winners and their neighbours survive the quantisation exactly
        for b, r in enumerate(reqs):
            assert torch.equal(pt["k_ref"][b], r.k.float())
    want = torch.cat([ar.saturated_expected(r, pt["v_ref"][b]) for b, r in enumerate(reqs)])
    H = KH * g
    args = (pt["q"], pt["ref_cache"], pt["qo"], pt["indices"], pt["indptr"], pt["last"], H, KH, D)
    ref64, _ = dense_attention_f64(*args, causal=causal, sm_scale=sm)
    assert ar.rows_equal(ref64.to(ar.BF), want, signed_zero=fp8), "the float64 reference itself"
    for ns in (1, 4):
        out = ar.emulate_paged(pt, KH, sm, causal=causal, nsplit=ns)
        assert ar.rows_equal(out, want, signed_zero=fp8), f"emulation x{ns}"
    # every placement class is reached by some row of the two requests
    won = set(int(x) for x in reqs[0].winner.flatten())
    if causal and n > 1:
        assert 1100 - 1 in won, "the key only the last token sees"
    parity_report(f"[attn-regime] saturated  D{D:<3d} n{n} g{g}{' fp8' if fp8 else ''}{'' if causal else ' non-causal'} sm_scale "
                  f"{_id(sm_scale):7s}: smallest winner gap {gap:.0f} log2 units, {len(won)} distinct winning keys in request 0")


def test_placements_cover_the_edges():
    p = ar.placements(2100, 4, 128)
    for want in (0, 31, 32, 33, 127, 128, 2099, 2096, 2048, 2047, 1056, 1055):
        assert want in p, want
    assert all(0 <= x < 2100 for x in p) and len(set(p)) == len(p)
    assert all(x < 33 for x in ar.placements(33, 4, 32))
