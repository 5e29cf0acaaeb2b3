"""The attention kernels beyond unit-variance scores, across every instantiation md_paged_attn can launch (-m gpu).

Inputs: tests/attn_regimes.py (wide, structured and saturated score regimes, non-default sm_scale, power-of-two fp8
scales); gate: tests/parity_util.check_attention, unchanged, on EVERY element against the float64 dense reference; the
saturated rows must equal the winning key's V row bit for bit (fp8 pages: -0 == +0); two guard rows after the output stay untouched.
tests/test_attn_regimes_cpu.py shows, without a GPU, that a correct implementation of the same algorithm stays inside
that gate on these inputs (max err/bound <= 0.70), so a failure here is a finding about the kernel.

Which case reaches which instantiation -- DERIVED FROM READING make_plan / launch_prefill in csrc/attn.hip, not asserted
at run time (the library exposes no "which kernel ran"):

  decode / verify: rows = n_max * g <= 32 -> paged_attn_kernel<D, QT, FP8, NWV> (+ attn_merge_kernel<D> when nsplit > 1)
    QT = 1 for rows <= 16, else 2; NWV = md_debug_set_attn_waves(4 | 8); nsplit = min(ceil(target_wgs / (B KH)),
    max_pages * page_size / 512, 64) with md_debug_set_attn_target_wgs and a 5120-key page-table bound -> 1, 2, 4, 10
    (at L = 33 eight of the ten splits are empty); "rule" = no knob, the tight bound.
      case                 D    rows (n x g)  QT  FP8  pages        every case: NWV 4 and 8, nsplit 1 / 2 / 4 / 10, rule
      d128-qt1-bf16-nhd    128  16 (4 x 4)    1   no   NHD 128
      d128-qt1-fp8-hnd     128   4 (1 x 4)    1   yes  HND 128
      d128-qt2-bf16-hnd    128  32 (4 x 8)    2   no   HND 128
      d128-qt2-fp8-nhd     128  20 (4 x 5)    2   yes  NHD 128
      d64-qt1-bf16-hnd      64  16 (4 x 4)    1   no   HND  32
      d64-qt1-fp8-nhd       64   4 (4 x 1)    1   yes  NHD 128
      d64-qt2-bf16-nhd      64  20 (4 x 5)    2   no   NHD 128
      d64-qt2-fp8-hnd       64  32 (4 x 8)    2   yes  HND 128
    = all 16 instantiations of paged_attn_kernel and both of attn_merge_kernel.

  prefill: rows > 32 -> QT = 2 for rows >= 128, else 1; NW = 8 only where rows >= 128 QT (md_debug_set_prefill_kt(kt, nw))
    prefill_attn_kernel<D, QT, FP8, NW, KT> with md_debug_set_prefill_mfma32(0) (fp8 and QT = 1 take it under every knob);
    KT = 64 only for bf16 D = 64 (md_debug_set_prefill_kt(64, .)); D = 128 is the TMASK (two compiled bodies) path,
    D = 64 the run-time mask path.  prefill32_attn_kernel<D, NW, KT, VP> for bf16 QT = 2: knob 32 / 64 / 128 / 129;
    128 keys only with 8 waves and 128-key pages, at either D (else 64; page 32 -> 32); 129 = <128, 8, 128, VP = false> at
    D = 128 with 8 waves and 128-key pages, and is halved to 64 (page 32: 32) otherwise.
      case                 D    rows          QT  FP8  NW    kernels reached
      p512-d128-bf16       128  512 (128x4)   2   no   4, 8  prefill<128,2,0,4|8,32>; prefill32<128,4|8,32|64>, <128,8,128,VP 1|0>
      p512-d64-bf16         64  512           2   no   4, 8  prefill<64,2,0,4|8,32|64>; prefill32<64,4|8,32|64>, <64,8,128>
      p512-d128-fp8        128  512           2   yes  4, 8  prefill<128,2,1,4|8,32>
      p512-d64-fp8          64  512           2   yes  4, 8  prefill<64,2,1,4|8,32>
      p512-d128-page32     128  512           2   no   4, 8  prefill32<128,4|8,32> (tile halved to the page), prefill<128,2,0,.,32>
      p100-d128-bf16       128  100 (100x1)   1   no   4     prefill<128,1,0,4,32>
      p100-d64-bf16         64  100           1   no   4     prefill<64,1,0,4,32|64>
      p100-d128-fp8        128  100           1   yes  4     prefill<128,1,1,4,32>
      p100-d64-fp8          64  100           1   yes  4     prefill<64,1,1,4,32>

Every case runs every regime of attn_regimes.REGIMES plus `saturated`, so no instantiation is left without a wide-range
case and a saturated case; sm_scale cycles through {default, 0.02, 0.25, 1.0} over (case, regime).  Every attention
knob of include/magicdec_hip_dev.h is called here, inside `with knobs(...)`, which restores every one on exit.
The saturated regime carries a trap key one past the causal limit of each of the last min(n - 1, 16) tokens of a chunk.
"""
import math

import pytest
import torch

from oracle import flashinfer_ref as fr
from tests import attn_regimes as ar
from tests.parity_util import check_attention, dense_attention_f64

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ALL_REGIMES = ar.REGIMES + ["saturated"]
SPLIT_KEYS = 5120          # page-table bound handed to the split rule: up to 10 KV splits


@pytest.fixture(scope="module")
def ops():
    from magicdec_amd import ops as _ops
    _ops._lib.load()      # fail loudly if the HIP library is missing
    return _ops


class knobs:
    """`with knobs(lib, waves=8, ...)`: set attention dev knobs, restore every one of them on exit."""

    def __init__(self, lib, target_wgs=0, waves=0, mfma32=-1, kt=64, nw=0):
        self.lib, self.v = lib, (target_wgs, waves, mfma32, kt, nw)

    def __enter__(self):
        t, w, m, kt, nw = self.v
        self.lib.md_debug_set_attn_target_wgs(t)
        self.lib.md_debug_set_attn_waves(w)
        self.lib.md_debug_set_prefill_mfma32(m)
        self.lib.md_debug_set_prefill_kt(kt, nw)

    def __exit__(self, *exc):
        self.lib.md_debug_set_attn_target_wgs(0)
        self.lib.md_debug_set_attn_waves(0)
        self.lib.md_debug_set_prefill_mfma32(-1)
        self.lib.md_debug_set_prefill_kt(64, 0)


def pick_scale(i, j):
    return ar.SM_SCALES[(i + j) % len(ar.SM_SCALES)]


def build_case(regime, ns, g, KH, D, lens, page_size, fp8, layout, sm_scale, seed):
    """Inputs, page table, oracle and float64 reference of one (case, regime): computed once per test, shared by every launch of it."""
    sm = ar.default_scale(D) if sm_scale is None else sm_scale
    scales = ar.pow2_scales(KH, seed) if fp8 else None
    if regime == "saturated":
        reqs = [ar.saturated_request(n, L, KH, g, D, seed + b, sm_scale, True, page_size, scales[0] if fp8 else None)
                for b, (n, L) in enumerate(zip(ns, lens))]
    else:
        reqs = [ar.make_request(regime, n, L, KH, g, D, seed + b, sm_scale) for b, (n, L) in enumerate(zip(ns, lens))]
        if fp8:
            ar.fit_fp8(reqs, scales[0])
    pt = ar.build_paged(reqs, page_size, seed, True, scales, layout)
    H = KH * g
    args = (pt["q"], pt["ref_cache"], pt["qo"], pt["indices"], pt["indptr"], pt["last"], H, KH, D)
    pt["oracle"] = fr.batch_prefill_paged(*args, causal=True, sm_scale=sm)
    pt["ref64"], pt["bnd"] = dense_attention_f64(*args, causal=True, sm_scale=sm)
    pt["sm"], pt["H"], pt["KH"], pt["D"] = sm, H, KH, D
    pt["want"] = None
    if regime == "saturated":
        pt["want"] = torch.cat([ar.saturated_expected(r, pt["v_ref"][b]) for b, r in enumerate(reqs)])
        if fp8:
            for b, r in enumerate(reqs):
                assert torch.equal(pt["k_ref"][b], r.k.float()), "saturated keys must survive the fp8 quantisation"
    return pt


def to_device(pt):
    d = {k: pt[k].to(DEV) for k in ("q", "qo", "indices", "indptr", "last", "dev_cache")}
    d["scales"] = tuple(s.to(DEV) for s in pt["scales"]) if pt["scales"] is not None else None
    return d


def launch(ops, pt, d, max_pages=None, sm=None, q=None, cache=None, scales=None):
    tot = pt["q"].shape[0]
    out = torch.full((tot + 2, pt["H"], pt["D"]), 7.0, dtype=BF, device=DEV)          # 2 guard rows
    ops.paged_attention(d["q"] if q is None else q, d["dev_cache"] if cache is None else cache, d["qo"], d["indices"],
                        d["indptr"], d["last"], pt["n_max"], max_pages or pt["max_pages"], ops.AttnWorkspace(DEV),
                        causal=True, sm_scale=pt["sm"] if sm is None else sm, out=out[:tot],
                        kv_scales=d["scales"] if scales is None else scales, kv_layout=pt["layout"])
    torch.cuda.synchronize()
    assert (out[tot:].float() == 7.0).all(), "wrote past the last query row"
    return out[:tot].cpu()


def gate(tag, pt, out):
    worst = check_attention(tag, out, pt["oracle"], pt["ref64"], pt["bnd"])
    if pt["want"] is not None:
        assert ar.rows_equal(out, pt["want"], signed_zero=pt["scales"] is not None), f"{tag}: a saturated row is not its winning key's V row"
    return worst


# ------------------------------------------------------------------------------------------ decode / verify
DECODE_CASES = [
    # name, D, n, g, KH, fp8, layout, lens, page size
    ("d128-qt1-bf16-nhd", 128, 4, 4, 2, False, "NHD", (2100, 1100), 128),
    ("d128-qt1-fp8-hnd", 128, 1, 4, 2, True, "HND", (2100, 33), 128),
    ("d128-qt2-bf16-hnd", 128, 4, 8, 1, False, "HND", (2100, 200), 128),
    ("d128-qt2-fp8-nhd", 128, 4, 5, 2, True, "NHD", (2100, 1100), 128),
    ("d64-qt1-bf16-hnd", 64, 4, 4, 2, False, "HND", (1100, 2100), 32),
    ("d64-qt1-fp8-nhd", 64, 4, 1, 2, True, "NHD", (2100, 200), 128),
    ("d64-qt2-bf16-nhd", 64, 4, 5, 2, False, "NHD", (2100, 33), 128),
    ("d64-qt2-fp8-hnd", 64, 4, 8, 1, True, "HND", (1100, 2100), 128),
]


@pytest.mark.parametrize("regime", ALL_REGIMES)
@pytest.mark.parametrize("case", DECODE_CASES, ids=[c[0] for c in DECODE_CASES])
def test_decode_verify_regimes_every_wave_and_split_count(ops, case, regime):
    """paged_attn_kernel with 4 and 8 waves and 1 / 2 / 4 / 10 KV splits (+ the rule's own choice) on the SAME inputs:
    every result inside the gate; the saturated rows bit-identical across all of them (each equals the V row)."""
    name, D, n, g, KH, fp8, layout, lens, ps = case
    ci, ri = [c[0] for c in DECODE_CASES].index(name), ALL_REGIMES.index(regime)
    pt = build_case(regime, (n,) * len(lens), g, KH, D, lens, ps, fp8, layout, pick_scale(ci, ri), 40 + ci)
    d = to_device(pt)
    lib = ops._lib.load()
    B = len(lens)
    outs = {"rule": launch(ops, pt, d)}
    for waves in (4, 8):
        for nsplit in (1, 2, 4, 10):
            with knobs(lib, target_wgs=256 if nsplit == 10 else nsplit * B * KH, waves=waves):
                outs[f"w{waves}-s{nsplit}"] = launch(ops, pt, d, max_pages=SPLIT_KEYS // ps)
    for k, o in outs.items():
        gate(f"{name} {regime} sm{pt['sm']:.3g} {k}", pt, o)


# ------------------------------------------------------------------------------------------ prefill
PREFILL_CASES = [
    # name, D, ns, g, KH, fp8, layout, lens, page size
    ("p512-d128-bf16", 128, (128, 100), 4, 2, False, "NHD", (700, 384), 128),
    ("p512-d64-bf16", 64, (128, 100), 4, 2, False, "HND", (700, 384), 128),
    ("p512-d128-fp8", 128, (128, 100), 4, 2, True, "HND", (700, 384), 128),
    ("p512-d64-fp8", 64, (128, 100), 4, 2, True, "NHD", (700, 384), 128),
    ("p512-d128-page32", 128, (128, 100), 4, 2, False, "NHD", (384, 700), 32),
    ("p100-d128-bf16", 128, (100, 40), 1, 2, False, "HND", (384, 200), 128),
    ("p100-d64-bf16", 64, (100, 40), 1, 2, False, "NHD", (384, 200), 128),
    ("p100-d128-fp8", 128, (100, 40), 1, 2, True, "NHD", (384, 200), 128),
    ("p100-d64-fp8", 64, (100, 40), 1, 2, True, "HND", (384, 200), 128),
]


def prefill_variants(D, ns, g, fp8):
    """(tag, mfma32, kt, nw) for every kernel the case can reach (see the module docstring)."""
    big = max(ns) * g >= 256
    nws = (4, 8) if big else (0,)
    kts = (32, 64) if (D == 64 and not fp8) else (64,)
    v = [("rule", -1, 64, 0)]
    v += [(f"16x16-kt{kt}-nw{nw}", 0, kt, nw) for kt in kts for nw in nws]
    if big and not fp8:
        v += [(f"32x32-{m}-nw{nw}", m, 64, nw) for m in (32, 64, 128, 129) for nw in nws]
    return v


@pytest.mark.parametrize("regime", ALL_REGIMES)
@pytest.mark.parametrize("case", PREFILL_CASES, ids=[c[0] for c in PREFILL_CASES])
def test_prefill_regimes_every_kernel_variant(ops, case, regime):
    """The 16x16 prefill kernel (32 / 64 keys per tile, 4 / 8 waves, compile-time and run-time mask, bf16 and fp8) and the
    32x32 kernel (knob 32 / 64 / 128 / 129, 4 / 8 waves) on the same inputs: lazy rescale under a moving and under a
    frozen maximum, scores far from zero, one winning key per row."""
    name, D, ns, g, KH, fp8, layout, lens, ps = case
    ci, ri = [c[0] for c in PREFILL_CASES].index(name), ALL_REGIMES.index(regime)
    pt = build_case(regime, ns, g, KH, D, lens, ps, fp8, layout, pick_scale(ci + 1, ri), 70 + ci)
    d = to_device(pt)
    lib = ops._lib.load()
    outs = {}
    for tag, m32, kt, nw in prefill_variants(D, ns, g, fp8):
        with knobs(lib, mfma32=m32, kt=kt, nw=nw):
            outs[tag] = launch(ops, pt, d)
    for k, o in outs.items():
        gate(f"{name} {regime} sm{pt['sm']:.3g} {k}", pt, o)


# ------------------------------------------------------------------------------------------ slots past the length
FAMILIES = {
    # name: (D, ns, g, KH, fp8, lens, knobs, page-table bound in keys)
    "decode-split4": (128, (4, 4), 4, 2, False, (2100, 1100), dict(target_wgs=16, waves=4), SPLIT_KEYS),
    "decode-qt2-8waves": (64, (4, 4), 8, 1, False, (1100, 200), dict(target_wgs=1, waves=8), None),
    "decode-fp8": (128, (4, 4), 5, 2, True, (1100, 200), dict(), None),
    "prefill16-tmask": (128, (128, 100), 4, 2, False, (700, 390), dict(mfma32=0), None),
    "prefill16-runtime-mask-kt64": (64, (128, 100), 4, 2, False, (700, 390), dict(mfma32=0, kt=64), None),
    "prefill16-fp8": (128, (100, 40), 1, 2, True, (390, 200), dict(), None),
    "prefill32-128keys": (128, (128, 100), 4, 2, False, (700, 390), dict(mfma32=128, nw=8), None),
    "prefill32-64keys-d64": (64, (128, 100), 4, 2, False, (700, 390), dict(mfma32=64, nw=4), None),
}


@pytest.mark.parametrize("layout", ["NHD", "HND"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_slots_past_last_page_len_never_reach_the_output(ops, family, layout):
    """The physical slots just past last_page_len inside the last MAPPED page (never past the mapping: nothing is read out
    of bounds) hold once a huge finite key that would win every row (with a huge V row), once NaN keys and Inf values:
    the output must be bit-identical to the run with those slots zeroed -- each kernel family, both layouts."""
    D, ns, g, KH, fp8, lens, kn, bound = FAMILIES[family]
    ps = 128
    pt = build_case("sink", ns, g, KH, D, lens, ps, fp8, layout, None, 90)
    d = to_device(pt)
    lib = ops._lib.load()
    nhd = pt["dev_cache"] if layout == "NHD" else pt["dev_cache"].permute(0, 1, 3, 2, 4)      # view [P, 2, slot, KH, D]
    u = ar.hadamard(D)[5]                   # the direction every query of the structured regimes carries

    def variant(kval, vval):
        c = nhd.float().clone()
        for b, L in enumerate(lens):
            pg = int(pt["indices"][int(pt["indptr"][b]) + (L - 1) // ps])
            assert L % ps != 0
            c[pg, 0, L % ps:] = kval if isinstance(kval, float) else kval.view(1, 1, D)
            c[pg, 1, L % ps:] = vval
        c = c.to(pt["dev_cache"].dtype)
        return (c if layout == "NHD" else c.permute(0, 1, 3, 2, 4)).contiguous().to(DEV)

    big = 448.0 if fp8 else 2.0 ** 100
    outs = {}
    with knobs(lib, **kn):
        mp = bound // ps if bound else None
        outs["zeroed"] = launch(ops, pt, d, max_pages=mp, cache=variant(0.0, 0.0))
        outs["huge"] = launch(ops, pt, d, max_pages=mp, cache=variant(u * big, big))
        outs["nan"] = launch(ops, pt, d, max_pages=mp, cache=variant(float("nan"), float("nan") if fp8 else float("inf")))
    gate(f"past-length {family} {layout}", pt, outs["zeroed"])
    for k in ("huge", "nan"):
        assert torch.equal(outs[k].view(torch.int16), outs["zeroed"].view(torch.int16)), f"{family} {layout}: {k} slots leaked"


# ------------------------------------------------------------------------------------------ sm_scale
@pytest.mark.parametrize("family", ["decode-split4", "decode-fp8", "prefill16-runtime-mask-kt64", "prefill16-tmask",
                                    "prefill32-128keys", "prefill16-fp8"])
def test_sm_scale_is_applied_exactly(ops, family):
    """The same inputs at two scales whose ratio is a power of two, q pre-multiplied on the host to compensate: every
    product q.k * sm_scale is the same float, so the outputs must be bit-identical -- and differ from the run that
    keeps q but not the scale (a kernel that ignored sm_scale would return that one)."""
    D, ns, g, KH, fp8, lens, kn, bound = FAMILIES[family]
    pt = build_case("ints4", ns, g, KH, D, lens, 128, fp8, "NHD", 0.25, 91)
    d = to_device(pt)
    lib = ops._lib.load()
    with knobs(lib, **kn):
        mp = bound // 128 if bound else None
        a = launch(ops, pt, d, max_pages=mp)
        b = launch(ops, pt, d, max_pages=mp, sm=0.25 / 8, q=(d["q"].float() * 8).to(BF))
        c = launch(ops, pt, d, max_pages=mp, sm=0.25 / 8)
    gate(f"sm_scale 0.25 {family}", pt, a)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "q * 8 at sm_scale / 8 must give identical products"
    assert not torch.equal(a.view(torch.int16), c.view(torch.int16)), "sm_scale has no effect"


@pytest.mark.parametrize("family", ["decode-fp8", "prefill16-fp8"])
@pytest.mark.parametrize("regime", ["ints4", "saturated"])
def test_fp8_k_scale_moves_into_sm_scale_and_back(ops, family, regime):
    """fp8 pages with non-monotonic power-of-two per-head scales: k_scale x 4 with sm_scale / 4 (and the reverse) is the
    same attention -- inside the gate each way, and the saturated rows equal bf16(byte * v_scale) for every head."""
    D, ns, g, KH, fp8, lens, kn, bound = FAMILIES[family]
    pt = build_case(regime, ns, g, KH, D, lens, 128, True, "NHD", None, 92)
    d = to_device(pt)
    ks, vs = d["scales"]
    for tag, f in (("as-is", 1.0), ("k_scale*4", 4.0), ("k_scale/4", 0.25)):
        out = launch(ops, pt, d, sm=pt["sm"] / f, scales=((ks * f).contiguous(), vs))
        gate(f"fp8 {family} {regime} {tag}", pt, out)


def test_plan_wrapper_forwards_sm_scale_to_the_kernel(ops):
    """Engine boundary: a non-default sm_scale given to PagedAttentionPlan.plan() reaches md_paged_attn -- the wrapper's
    result equals a direct call with that scale and differs from the default-scale one."""
    from magicdec_amd import mylib_ops
    D, ns, g, KH, fp8, lens, kn, bound = FAMILIES["decode-qt2-8waves"]
    pt = build_case("ints2", ns, g, KH, D, lens, 128, False, "NHD", 0.25, 93)
    d = to_device(pt)
    w = mylib_ops.PagedAttentionPlan(None, "NHD")
    w.plan(d["qo"], d["indptr"], d["indices"], d["last"], pt["H"], KH, D, 128, q_data_type=BF, causal=True, sm_scale=0.25)
    got = w.run(d["q"], d["dev_cache"]).cpu()
    direct = launch(ops, pt, d)
    default = launch(ops, pt, d, sm=1.0 / math.sqrt(D))
    gate("plan-wrapper sm_scale 0.25", pt, got)
    assert torch.equal(got.view(torch.int16), direct.view(torch.int16))
    assert not torch.equal(got.view(torch.int16), default.view(torch.int16))
