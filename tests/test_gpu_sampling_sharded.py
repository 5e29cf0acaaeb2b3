"""GPU tests of the vocab-sharded sampling phases (csrc/sample.hip, include/magicdec_hip.h K11 "sharded") through the C
ABI, with W ranks emulated in ONE process: rank r gets the column slice [off_r, off_r + V_r) of every logits row (a view
of the full tensor, row stride V), its own counters, ring shard and stats; the all-reduce between two phases is a
stack(...).amax(0) / .sum(0) over the ranks' buffers.

The claim under test is an equality, not a tolerance: tokens, ring_stats, target_stats, ring contents and counters of
the sharded chain are the BITS of ops.sample_rows / ops.spec_verify_sample on the whole rows with the same seed and
counters (those kernels are pinned to the numpy restatement by tests/test_gpu_sampling.py).  On the small cases the
sharded outputs are also given to the admissible-outcome oracle (tests/sampling_cases.check_iteration) directly."""
import math
import random

import numpy as np
import pytest
import torch

from magicdec_amd import ops
from tests import sampling_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I64 = dict(dtype=torch.int64, device=DEV)


def _widths(V, W):
    """torch.chunk's split (Engine/tp.py shards the lm head with it): the last rank may get fewer columns."""
    c = -(-V // W)
    return [min(c, V - i * c) for i in range(W) if V - i * c > 0]


def _offsets(widths):
    return [sum(widths[:i]) for i in range(len(widths))]


def _counters(it):
    c = torch.zeros(4, dtype=torch.int32, device=DEV)
    c[0] = it
    return c


def _stats_np(st):
    a = st.cpu().numpy().reshape(-1, 2)
    lo = a[:, 0].astype(np.int64).view(np.uint64)
    return ((lo & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32), (lo >> np.uint64(32)).astype(np.uint32),
            a[:, 1].view(np.uint64))


def _dev_rows(x2d, pad):
    if pad is None:
        return x2d.contiguous().to(DEV)
    off, extra = pad
    rows, V = x2d.shape
    full = torch.full((rows, off + V + extra), 60.0, dtype=torch.bfloat16, device=DEV)
    full[:, off:off + V] = x2d.to(DEV)
    return full[:, off:off + V]


def _all_reduce(bufs, op):
    red = torch.stack(bufs).amax(0) if op == "max" else torch.stack(bufs).sum(0)
    for b in bufs:
        b.copy_(red)


class _Ranks:
    """The per-rank state of W emulated ranks and the two logical calls as phase chains."""

    def __init__(self, V, widths, B, G, T, top_p, seed, it, full_ring=False):
        self.V, self.widths, self.offs, self.W = V, widths, _offsets(widths), len(widths)
        assert sum(widths) == V
        self.B, self.G, self.T, self.top_p, self.seed = B, G, T, top_p, seed
        self.full_ring = full_ring
        self.ctr = [_counters(it) for _ in widths]
        self.ring = [torch.zeros((B, G, V if full_ring else w), dtype=torch.bfloat16, device=DEV) for w in widths]
        self.rst = [torch.zeros((B, G, 2), **I64) for _ in widths]
        self.tst = [torch.zeros((B * (G + 1), 2), **I64) for _ in widths]
        self.collectives = 0

    def _reduce(self, bufs, op):
        self.collectives += 1
        _all_reduce(bufs, op)

    def _shards(self, x):
        return [x[:, o:o + w] for o, w in zip(self.offs, self.widths)]

    def _filter(self, xs, n, R, extra, row_sel=None, **probe):
        rk = range(self.W)
        red = [torch.zeros(R + extra, **I64) for _ in rk]
        for r in rk:
            kw = {k: v[r] if isinstance(v, list) else v for k, v in probe.items()}
            ops.shard_max(xs[r], n, self.offs[r], self.V, red[r], row_sel=row_sel, **kw)
        self._reduce(red, "max")
        hi = [torch.zeros((R, 256), **I64) for _ in rk]
        for r in rk:
            ops.shard_hist(xs[r], n, self.T, self.top_p, red[r], hi[r], row_sel=row_sel)
        self._reduce(hi, "sum")
        lo = [None] * self.W
        if self.top_p < 1:
            lo = [torch.zeros((R, 256), **I64) for _ in rk]
            for r in rk:
                ops.shard_hist(xs[r], n, self.T, self.top_p, red[r], lo[r], hist_hi=hi[r], row_sel=row_sel)
            self._reduce(lo, "sum")
        return red, hi, lo

    def draw(self, x, n, purpose, advance, row_sel=None, draft=True):
        """One logical md_sample_rows on the full rows x [B*n, V] -> tokens [B, n] (asserted equal on every rank)."""
        self.collectives = 0
        xs = self._shards(x)
        red, hi, lo = self._filter(xs, n, self.B, 0, row_sel=row_sel)
        cand = [torch.zeros(self.B, **I64) for _ in range(self.W)]
        for r in range(self.W):
            ops.shard_draw(xs[r], n, self.offs[r], self.V, self.T, self.top_p, self.seed, purpose, self.ctr[r], red[r],
                           hi[r], lo[r], cand[r], row_sel=row_sel, ring=self.ring[r] if draft else None,
                           ring_stats=self.rst[r] if draft else None)
        self._reduce(cand, "max")
        toks = [ops.shard_finish(cand[r], n, self.ctr[r], advance) for r in range(self.W)]
        assert self.collectives == (4 if self.top_p < 1 else 3)
        for t in toks[1:]:
            assert torch.equal(t, toks[0])
        return toks[0]

    def verify(self, x, tb):
        """One logical md_spec_verify_sample on the full rows x [B*(G+1), V] -> target_tokens [B, G+1]."""
        self.collectives = 0
        xs = self._shards(x)
        B, G = self.B, self.G
        # the ring a rank reads: its shard, or its columns of a full ring -- by column offset (even ranks) or as a view
        rings, coff = [], []
        for r in range(self.W):
            if not self.full_ring:
                rings.append(self.ring[r]), coff.append(0)
            elif r % 2 == 0:
                rings.append(self.ring[r]), coff.append(self.offs[r])
            else:
                rings.append(self.ring[r][:, :, self.offs[r]:self.offs[r] + self.widths[r]]), coff.append(0)
        red, hi, lo = self._filter(xs, 1, B * (G + 1), B * G, tokens_buffer=tb, ring=rings, ring_col_offset=coff)
        cand = [torch.zeros((B, 3), **I64) for _ in range(self.W)]
        for r in range(self.W):
            ops.spec_verify_shard(xs[r], tb, self.offs[r], self.V, rings[r], self.rst[r], red[r], hi[r], lo[r],
                                  self.tst[r], self.ctr[r], self.T, self.top_p, self.seed, cand[r],
                                  ring_col_offset=coff[r])
        self._reduce(cand, "max")
        tts = [ops.spec_verify_shard_finish(cand[r], tb, self.ctr[r]) for r in range(self.W)]
        assert self.collectives == (4 if self.top_p < 1 else 3)
        for t in tts[1:]:
            assert torch.equal(t, tts[0])
        return tts[0]


def _reference_iteration(c, tokens_edit=None):
    """The iteration of case `c` by the one-GPU kernels (the reference of every test here)."""
    V, B, G, T, top_p, seed = c["V"], c["B"], c["G"], c["T"], c["top_p"], c["seed"]
    ctr = _counters(c["it"])
    ring = torch.zeros((B, G, V), dtype=torch.bfloat16, device=DEV)
    rst = torch.zeros((B, G, 2), **I64)
    tst = torch.zeros((B * (G + 1), 2), **I64)
    tb = torch.zeros((B, G + 1), **I64)
    tb[:, 0] = c["tok0"].to(DEV)
    sel = c["row_sel"].to(DEV) if c["row_sel"] is not None else None
    for j, x in enumerate(c["dl"]):
        n = x.shape[1]
        t = ops.sample_rows(_dev_rows(x.reshape(B * n, V), c["pad"]), n, T, top_p, seed, ops.SAMPLE_DRAFT, ctr,
                            ops.ADVANCE_STEP, row_sel=sel if n == 2 else None, ring=ring, ring_stats=rst)
        tb[:, j + 1] = t[:, 0]
    drafts = tb[:, 1:].clone()
    if tokens_edit is not None:
        tokens_edit(tb)
    tt = ops.spec_verify_sample(_dev_rows(c["tl"].reshape(B * (G + 1), V), c["pad"]), tb, ring, rst, tst, ctr, T, top_p,
                                seed)
    torch.cuda.synchronize()
    return dict(ring=ring, rst=rst, tst=tst, drafts=drafts, tb=tb, tt=tt, ctr=ctr)


def _sharded_iteration(c, widths, tokens_edit=None, full_ring=False):
    V, B, G = c["V"], c["B"], c["G"]
    rk = _Ranks(V, widths, B, G, c["T"], c["top_p"], c["seed"], c["it"], full_ring=full_ring)
    tb = torch.zeros((B, G + 1), **I64)
    tb[:, 0] = c["tok0"].to(DEV)
    sel = c["row_sel"].to(DEV) if c["row_sel"] is not None else None
    for j, x in enumerate(c["dl"]):
        n = x.shape[1]
        xd = _dev_rows(x.reshape(B * n, V), c["pad"])
        if full_ring:       # --replicate_draft: every rank runs the whole draft and the one-GPU draw
            toks = [ops.sample_rows(xd, n, c["T"], c["top_p"], c["seed"], ops.SAMPLE_DRAFT, rk.ctr[r], ops.ADVANCE_STEP,
                                    row_sel=sel if n == 2 else None, ring=rk.ring[r], ring_stats=rk.rst[r])
                    for r in range(rk.W)]
            t = toks[0]
        else:
            t = rk.draw(xd, n, ops.SAMPLE_DRAFT, ops.ADVANCE_STEP, row_sel=sel if n == 2 else None)
        assert bool((t == t[:, :1]).all())
        tb[:, j + 1] = t[:, 0]
    for ctr in rk.ctr:
        assert ctr.tolist() == [c["it"], G, 0, 0]
    drafts = tb[:, 1:].clone()
    if tokens_edit is not None:
        tokens_edit(tb)
    tt = rk.verify(_dev_rows(c["tl"].reshape(B * (G + 1), V), c["pad"]), tb)
    torch.cuda.synchronize()
    return dict(rk=rk, drafts=drafts, tb=tb, tt=tt)


def _assert_same(c, widths, tokens_edit=None, full_ring=False, oracle=False):
    ref = _reference_iteration(c, tokens_edit)
    got = _sharded_iteration(c, widths, tokens_edit, full_ring)
    rk, tag = got["rk"], f"{c['name']} widths={widths}"
    assert torch.equal(got["drafts"], ref["drafts"]), f"{tag}: draft tokens"
    assert torch.equal(got["tt"], ref["tt"]), f"{tag}: target_tokens {got['tt'].tolist()} vs {ref['tt'].tolist()}"
    for r in range(rk.W):
        assert torch.equal(rk.rst[r], ref["rst"]), f"{tag}: ring_stats of rank {r}"
        assert torch.equal(rk.tst[r], ref["tst"]), f"{tag}: target_stats of rank {r}"
        assert torch.equal(rk.ctr[r], ref["ctr"]), f"{tag}: counters of rank {r}"
        cols = ref["ring"] if full_ring else ref["ring"][:, :, rk.offs[r]:rk.offs[r] + widths[r]]
        assert torch.equal(rk.ring[r].view(torch.int16), cols.contiguous().view(torch.int16)), f"{tag}: ring of rank {r}"
    assert ref["ctr"].tolist() == [c["it"] + 1, 0, 0, 0]
    if oracle:
        ring = torch.cat([x.cpu() for x in rk.ring], dim=2) if not full_ring else rk.ring[0].cpu()
        sc.check_iteration(c, sc.bits_of(ring), _stats_np(rk.rst[0]), _stats_np(rk.tst[0]), got["drafts"].cpu().numpy(),
                           got["tt"].cpu().numpy(), got["tb"].cpu().numpy())
    return ref, got


SHAPES = [("v1001_w3", 1001, 3, 6, 3), ("v2048_w2", 2048, 2, 6, 3), ("v2048_w8", 2048, 8, 6, 3),
          ("v151936_w8_1024threads", 151936, 8, 4, 3), ("v128256_w8_256threads", 128256, 8, 4, 3)]


@pytest.mark.parametrize("T", [0.6, 1.5])
@pytest.mark.parametrize("top_p", [1.0, 0.9, 0.05])
@pytest.mark.parametrize("name,V,W,B,G", SHAPES)
def test_sharded_iteration_is_bit_identical_to_one_gpu(name, V, W, B, G, top_p, T):
    """1001 / 3 = 334, 334, 333: odd offsets, unaligned rows, noise groups of 4 straddling a shard border; 151936 / 8 =
    18992 columns run the 1024-thread kernels, 128256 / 8 = 16032 the 256-thread ones."""
    widths = _widths(V, W)
    assert len(widths) == W
    if V == 1001:
        assert widths == [334, 334, 333]
    c = sc.random_case(f"{name}_{top_p}_{T}", V, B, G, T, top_p, 0.5)
    _assert_same(c, widths, oracle=V <= 2048)


@pytest.mark.parametrize("top_p", [1.0, 0.9])
def test_one_rank_equals_the_plain_path(top_p):
    c = sc.random_case(f"w1_{top_p}", 1001, 5, 2, 0.8, top_p, 0.7)
    _assert_same(c, [1001], oracle=True)


@pytest.mark.parametrize("V,W", [(1001, 3), (2048, 8)])
def test_two_token_draft_step_with_mixed_row_selection(V, W):
    _assert_same(_case_two_token(V), _widths(V, W), oracle=True)


def _planted(name, V, B, G, T, top_p, plant, sigma=0.5):
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    tl = torch.randn(B, G + 1, V, generator=g) * 2.0
    dl = tl[:, :G] + torch.randn(B, G, V, generator=g) * sigma
    plant(tl, dl)
    return sc.custom_case(name, tl, dl, T, top_p)


W3 = [334, 334, 333]                          # torch.chunk of 1001 columns over three ranks


def _case_boundary_elsewhere():
    def plant(tl, dl):
        for x in (tl, dl):
            x.fill_(-30.0)
            x[:, :, 5] = 4.0
            x[:, :, 700:732] = torch.linspace(3.0, 2.0, 32)
            x[:, :, 400] = -1.0
    return _planted("boundary_elsewhere", 1001, 4, 2, 1.0, 0.9, plant)


def _case_neginf_shard(top_p):
    def plant(tl, dl):
        tl[:, :, 334:668] = float("-inf")
        dl[:, :, 334:668] = float("-inf")
        tl[1, :, 668:] = float("-inf")          # and a request with two empty shards
        dl[1, :, 668:] = float("-inf")
    return _planted(f"neginf_shard_{top_p}", 1001, 4, 2, 0.6, top_p, plant)


def _case_tie_split(top_p):
    def plant(tl, dl):
        for x in (tl, dl):
            x.fill_(float("-inf"))
            x[:, :, 0] = 2.0
            x[:, :, 330:338] = 0.0
    return _planted(f"tie_split_{top_p}", 1001, 3, 2, 1.0, top_p, plant, sigma=0.0)


def _case_draft_last_shard():
    V = 2048

    def plant(tl, dl):
        tl[:, :, 3] += 12.0                     # the target is peaked on rank 0
        dl[:, :, V - 1] += 12.0                 # the draft on the last rank
    return _planted("draft_last_shard", V, 6, 3, 0.6, 0.9, plant)


def _case_fallback():
    """-> (case, the edit of the tokens_buffer the verify reads)"""
    def plant(tl, dl):
        tl[:, :, 10:20] += 8.0
        tl[:, :, 1000] = -40.0
        dl.copy_(tl[:, :dl.shape[1]])

    def edit(tb):
        tb[:, 1] = 1000
        tb[2, 1] = 12                           # ... and a request whose rejected d is in the kept set's rank
    return _planted("fallback_sharded", 1001, 4, 2, 0.7, 0.5, plant, sigma=0.0), edit


def _case_two_token(V):
    B, G = 6, 3
    c = sc.random_case(f"two_token_{V}", V, B, G, 0.6, 0.9, 0.5)
    g = torch.Generator().manual_seed(V)
    row_sel = torch.tensor([1, 2] * (B // 2))
    other = (torch.randn(B, 1, V, generator=g) * 2.5).to(sc.BF)
    first = torch.where((row_sel == 1).view(B, 1, 1), c["dl"][0], other)
    second = torch.where((row_sel == 2).view(B, 1, 1), c["dl"][0], other)
    c["dl"][0] = torch.cat([first, second], dim=1).contiguous()
    c["row_sel"] = row_sel
    return c


def oracle_cases():
    """Every case of this file that is also given to the oracle -> (case, tokens edit or None); what
    tests/test_sampling_sharded_cpu.py requires to be unambiguous for it."""
    for name, V, W, B, G in SHAPES:
        if V <= 2048:
            for top_p in (1.0, 0.9, 0.05):
                for T in (0.6, 1.5):
                    yield sc.random_case(f"{name}_{top_p}_{T}", V, B, G, T, top_p, 0.5), None
    for top_p in (1.0, 0.9):
        yield sc.random_case(f"w1_{top_p}", 1001, 5, 2, 0.8, top_p, 0.7), None
    for V in (1001, 2048):
        yield _case_two_token(V), None
        yield sc.random_case(f"replicate_{V}", V, 6, 3, 0.6, 0.9, 0.5), None
    yield _case_boundary_elsewhere(), None
    for top_p in (0.9, 1.0):
        yield _case_neginf_shard(top_p), None
    for top_p in (0.5, 0.4):
        yield _case_tie_split(top_p), None
    yield _case_draft_last_shard(), None
    yield _case_fallback()
    yield sc.random_case("bonus_sharded", 2048, 6, 3, 0.8, 0.9, 0.0), None
    for i in range(10):
        c = _fuzz_case(i)[0]
        if c["V"] <= 2048:
            yield c, None


def test_top_p_boundary_bin_wholly_on_another_rank():
    """The maximum (and most of the mass) sits on rank 0, the tokens around the top-p boundary on rank 2: rank 0 and 1
    contribute zeros to the low-byte histogram of the boundary bin."""
    _assert_same(_case_boundary_elsewhere(), W3, oracle=True)


def test_a_shard_that_is_minus_infinity_throughout():
    for top_p in (0.9, 1.0):
        _assert_same(_case_neginf_shard(top_p), W3, oracle=True)


@pytest.mark.parametrize("top_p", [0.5, 0.4])
def test_tie_group_at_the_boundary_split_across_two_shards(top_p):
    """Token 0 holds e^2 / (e^2 + 8) = 0.48 of the mass, a tie group of 8 tokens the rest, half of it on each side of
    the border at 334: top_p 0.5 keeps the group (0.48 <= 0.5), top_p 0.4 drops it -- whole, on both ranks."""
    ref, got = _assert_same(_case_tie_split(top_p), W3, oracle=True)
    _, kstar, _ = _stats_np(got["rk"].tst[0])
    assert (kstar == (0x8000 if top_p == 0.5 else 0xC000)).all()    # key(+0.0): the group is kept; key(2.0): dropped


def test_draft_token_on_the_last_shard_and_residual_winner_elsewhere():
    V = 2048
    ref, got = _assert_same(_case_draft_last_shard(), _widths(V, 8), oracle=True)
    assert (got["drafts"][:, 0] == V - 1).all() and (got["tt"][:, 0] == 3).all()


def test_out_of_range_draft_tokens_are_rejections_owned_by_no_rank():
    V, widths = 1001, [334, 334, 333]
    c = sc.random_case("oor_sharded", V, 6, 3, 0.8, 0.9, 0.0)

    def edit(tb):
        tb[0, 1] = V
        tb[1, 2] = -3
        tb[2, 3] = 2 ** 40
        tb[3, 1] = 2 ** 31 + 5
    ref, got = _assert_same(c, widths, tokens_edit=edit)
    tt = got["tt"].cpu()
    assert tt[0, 1:].tolist() == [-1, -1, -1] and tt[1, 2:].tolist()[1:] == [-1] and 0 <= tt[0, 0] < V


def test_zero_residual_fallback_with_d_and_the_winner_on_different_shards():
    """draft row == target row and a draft token outside the kept set: p~(d) = q~(d) = 0 rejects it, the residual is 0
    everywhere, the token comes from p~ without d.  d is planted on the last rank, the mass on rank 0."""
    c, edit = _case_fallback()
    ref, got = _assert_same(c, W3, tokens_edit=edit, oracle=True)
    tt = got["tt"].cpu()
    assert (tt[[0, 1, 3], 1] == -1).all() and ((tt[[0, 1, 3], 0] >= 10) & (tt[[0, 1, 3], 0] < 20)).all()


def test_every_draft_accepted_gives_the_bonus_draw():
    V = 2048
    c = sc.random_case("bonus_sharded", V, 6, 3, 0.8, 0.9, 0.0)
    for W in (2, 8):
        ref, got = _assert_same(c, _widths(V, W), oracle=True)
        assert torch.equal(got["tt"][:, :3], got["drafts"]) and (got["tt"][:, 3] >= 0).all()


def test_end_of_text_case_through_the_accept_kernel():
    """The verify's output feeds the unchanged accept kernel: same target_tokens -> same cut at an end-of-text draft."""
    c, eot_1, eot_2, expect = sc.eot_case()
    ref, got = _assert_same(c, _widths(c["V"], 3))
    assert expect
    B, G = c["B"], c["G"]
    assert torch.equal(got["tt"][:, :G], got["drafts"])            # ring == target: every draft is accepted
    i32 = dict(dtype=torch.int32, device=DEV)
    out, num_nodes = torch.zeros((B, 64), **I64), torch.full((B,), 20, **I64)
    cachelens, lpl = torch.full((B,), 20 + G + 1, **i32), torch.full((B,), 20 + G + 1, **i32)
    an, bonus, dbl, cu = torch.zeros(B, **I64), torch.zeros(B, **I64), torch.zeros((B, 2), **I64), torch.ones(B, **I64)
    flags = torch.zeros(2, **i32)
    ops.accept_rollback(got["tb"].clone(), got["tt"], out, num_nodes, cachelens, lpl, None, None, G, G, G, eot_1, eot_2,
                        10 ** 6, an, bonus, dbl, cu, flags)
    torch.cuda.synchronize()
    drafts = got["drafts"].cpu().numpy()
    for b in range(B):
        eot = [j for j in range(G) if drafts[b, j] in (eot_1, eot_2)]
        assert int(an[b]) == (eot[0] + 1 if eot else G + 1), (b, drafts[b], int(an[b]))


@pytest.mark.parametrize("V,W", [(1001, 3), (2048, 2)])
def test_replicated_draft_layout_reads_its_columns_of_a_full_ring(V, W):
    c = sc.random_case(f"replicate_{V}", V, 6, 3, 0.6, 0.9, 0.5)
    _assert_same(c, _widths(V, W), full_ring=True, oracle=True)


FUZZ_V, FUZZ_W = [50, 1001, 2048, 32003], [2, 3, 4, 8]


def _fuzz_case(i):
    r = random.Random(7100 + i)
    V, W = FUZZ_V[i % 4], FUZZ_W[(i // 4 + i) % 4]
    B, G = r.randint(1, 6), r.randint(1, 4)
    T = math.exp(r.uniform(math.log(0.2), math.log(3.0)))
    top_p = 1.0 if r.random() < 0.3 else r.uniform(0.05, 0.99)
    sigma = r.choice([0.0, 0.2, 0.5, 1.0, 2.0])
    if r.random() < 0.5:                        # uneven widths at random cut points
        cuts = sorted(r.sample(range(1, V), W - 1))
        widths = [b - a for a, b in zip([0] + cuts, cuts + [V])]
    else:
        widths = _widths(V, W)
    g = torch.Generator().manual_seed(7100 + i)
    tl = torch.randn(B, G + 1, V, generator=g) * r.choice([0.5, 1.5, 2.5, 4.0])
    dl = tl[:, :G] + torch.randn(B, G, V, generator=g) * sigma
    for _ in range(r.randint(0, 3)):
        b, j, kind = r.randrange(B), r.randrange(G), r.choice(["ties", "neginf", "peak"])
        if kind == "ties":
            idx = torch.randperm(V, generator=g)[: r.randint(2, max(2, V // 3))]
            val = float(tl[b, j].max()) - r.choice([0.0, 0.5, 2.0])
            tl[b, j, idx] = val
            dl[b, j, idx] = val
        elif kind == "neginf":
            a = r.randrange(V)
            e = min(V, a + r.randint(1, max(1, V // 2)))
            tl[b, j, a:e] = float("-inf")
            dl[b, j, a:e] = float("-inf")
            if a == 0 and e == V:
                tl[b, j, 0] = dl[b, j, 0] = 0.0
        else:
            v = r.randrange(V)
            tl[b, j, v] = dl[b, j, v] = float(tl[b, j][torch.isfinite(tl[b, j])].max()) + 3.0
    pad = None if r.random() < 0.5 else (r.choice([0, 3, 8]), r.choice([5, 8, 64]))
    c = sc.custom_case(f"shardfuzz{i}", tl, dl, T, top_p, it=r.randint(0, 2 ** 30), pad=pad, seed=r.getrandbits(64),
                       restate=sc.subset(B, 3, i))
    c["tok0"] = torch.randint(0, V, (B,), generator=g)
    return c, widths


@pytest.mark.parametrize("i", range(10))
def test_seeded_fuzz_family(i):
    c, widths = _fuzz_case(i)
    _assert_same(c, widths, oracle=c["V"] <= 2048)


def test_prefill_and_baseline_draws_advance_the_iteration():
    V, widths, B = 1001, [334, 334, 333], 5
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(B * 3, V, generator=g) * 2).to(sc.BF).to(DEV)
    for purpose in (ops.SAMPLE_PREFILL, ops.SAMPLE_BASELINE):
        ctr = _counters(9)
        ref = ops.sample_rows(x, 3, 0.7, 0.9, 42, purpose, ctr, ops.ADVANCE_ITER)
        rk = _Ranks(V, widths, B, 1, 0.7, 0.9, 42, 9)
        got = rk.draw(x, 3, purpose, ops.ADVANCE_ITER, draft=False)
        assert torch.equal(got, ref)
        for c in rk.ctr:
            assert torch.equal(c, ctr) and c.tolist() == [10, 0, 0, 0]


def test_sharded_phases_reject_bad_arguments():
    V, w, B, G = 64, 32, 2, 2
    x = torch.zeros((B * (G + 1), w), dtype=torch.bfloat16, device=DEV)
    red = torch.zeros(B * (G + 1) + B * G, **I64)
    hi = torch.zeros((B * (G + 1), 256), **I64)
    ring = torch.zeros((B, G, w), dtype=torch.bfloat16, device=DEV)
    rst = torch.zeros((B, G, 2), **I64)
    tst = torch.zeros((B * (G + 1), 2), **I64)
    tb = torch.zeros((B, G + 1), **I64)
    ctr = _counters(0)
    cand = torch.zeros((B, 3), **I64)
    with pytest.raises(ValueError, match="inside the vocabulary"):
        ops.shard_max(x, 1, 40, V, red[:B * (G + 1)].contiguous())               # 40 + 32 > 64
    with pytest.raises(ValueError, match="inside the vocabulary"):
        ops.shard_max(x, 1, -1, V, red[:B * (G + 1)].contiguous())
    with pytest.raises(ValueError, match="red"):
        ops.shard_max(x, 1, 0, V, red[:3].contiguous())
    with pytest.raises(ValueError, match="ring"):
        ops.shard_max(x, 1, 0, V, red, tokens_buffer=tb)                           # a probe without a ring
    with pytest.raises(ValueError, match="exceed"):
        ops.shard_max(x, 1, 32, V, red, tokens_buffer=tb, ring=ring, ring_col_offset=32)
    with pytest.raises(ValueError, match="low-byte"):
        ops.shard_hist(x, 1, 1.0, 1.0, red, hi.clone(), hist_hi=hi)
    with pytest.raises(ValueError, match="go together"):
        ops.shard_draw(x[:B], 1, 0, V, 1.0, 1.0, 1, ops.SAMPLE_DRAFT, ctr, red[:B].contiguous(), hi[:B].contiguous(),
                       None, cand[:, 0].contiguous(), ring=ring)                  # ring without stats
    with pytest.raises(ValueError, match="low-byte"):
        ops.shard_draw(x[:B], 1, 0, V, 1.0, 0.9, 1, ops.SAMPLE_BASELINE, ctr, red[:B].contiguous(), hi[:B].contiguous(),
                       None, cand[:, 0].contiguous())
    with pytest.raises(ValueError, match="inside the vocabulary"):
        ops.spec_verify_shard(x, tb, 33, V, ring, rst, red, hi, None, tst, ctr, 1.0, 1.0, 1, cand)
    with pytest.raises(ValueError, match="cand"):
        ops.spec_verify_shard(x, tb, 0, V, ring, rst, red, hi, None, tst, ctr, 1.0, 1.0, 1, cand[:, :2].contiguous())
    with pytest.raises(ValueError, match="temperature"):
        ops.shard_hist(x, 1, 0.0, 1.0, red, hi)
    # the library's own checks (the wrappers above are the first line only)
    from magicdec_amd import _lib
    lib = _lib.load()
    p = lambda t: t.data_ptr()
    assert lib.md_sample_shard_max(p(x), w, B * (G + 1), 1, w, None, None, None, 0, 0, 0, 40, V, p(red), None) != 0
    assert lib.md_sample_shard_draw(p(x), w, B, 1, w, 0, V, 1.0, 1.0, 1, ops.SAMPLE_DRAFT, None, p(ctr), p(red), p(hi),
                                    None, p(ring), None, G, p(cand), None) != 0
    assert ctr.tolist() == [0, 0, 0, 0]


def test_captured_graph_of_the_local_phases_replays_the_eager_result():
    """One rank (the all-reduce is the identity), the whole chain of a draft draw and of a verify in one graph each:
    the counters are read on the device, so the replays walk the same stream as eager calls."""
    V, B, G, T, top_p, seed = 2048, 4, 2, 0.8, 0.9, 77
    c = sc.random_case("graph_sharded", V, B, G, T, top_p, 0.6)
    xs = [c["dl"][j].reshape(B, V).to(DEV) for j in range(G)]
    xt = c["tl"].reshape(B * (G + 1), V).to(DEV)

    def state():
        return dict(ctr=_counters(5), ring=torch.zeros((B, G, V), dtype=torch.bfloat16, device=DEV),
                    rst=torch.zeros((B, G, 2), **I64), tst=torch.zeros((B * (G + 1), 2), **I64),
                    tb=torch.zeros((B, G + 1), **I64), red=torch.zeros(B, **I64), hi=torch.zeros((B, 256), **I64),
                    lo=torch.zeros((B, 256), **I64), cand=torch.zeros(B, **I64), tok=torch.zeros((B, 1), **I64),
                    vred=torch.zeros(B * (G + 1) + B * G, **I64), vhi=torch.zeros((B * (G + 1), 256), **I64),
                    vlo=torch.zeros((B * (G + 1), 256), **I64), vcand=torch.zeros((B, 3), **I64),
                    tt=torch.zeros((B, G + 1), **I64), x=torch.zeros((B, V), dtype=torch.bfloat16, device=DEV))

    def draft(s):
        ops.shard_max(s["x"], 1, 0, V, s["red"])
        ops.shard_hist(s["x"], 1, T, top_p, s["red"], s["hi"])
        ops.shard_hist(s["x"], 1, T, top_p, s["red"], s["lo"], hist_hi=s["hi"])
        ops.shard_draw(s["x"], 1, 0, V, T, top_p, seed, ops.SAMPLE_DRAFT, s["ctr"], s["red"], s["hi"], s["lo"], s["cand"],
                       ring=s["ring"], ring_stats=s["rst"])
        ops.shard_finish(s["cand"], 1, s["ctr"], ops.ADVANCE_STEP, out=s["tok"])

    def verify(s):
        ops.shard_max(xt, 1, 0, V, s["vred"], tokens_buffer=s["tb"], ring=s["ring"])
        ops.shard_hist(xt, 1, T, top_p, s["vred"], s["vhi"])
        ops.shard_hist(xt, 1, T, top_p, s["vred"], s["vlo"], hist_hi=s["vhi"])
        ops.spec_verify_shard(xt, s["tb"], 0, V, s["ring"], s["rst"], s["vred"], s["vhi"], s["vlo"], s["tst"], s["ctr"],
                              T, top_p, seed, s["vcand"])
        ops.spec_verify_shard_finish(s["vcand"], s["tb"], s["ctr"], out=s["tt"])

    def iterations(s, run_draft, run_verify):
        outs = []
        for _ in range(2):
            for j in range(G):
                s["x"].copy_(xs[j])
                run_draft()
                s["tb"][:, j + 1] = s["tok"][:, 0]
            run_verify()
            torch.cuda.synchronize()
            outs.append((s["tb"].clone(), s["tt"].clone(), s["rst"].clone(), s["tst"].clone(), s["ctr"].clone()))
        return outs

    e = state()
    eager = iterations(e, lambda: draft(e), lambda: verify(e))
    s = state()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        draft(s), verify(s)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gd, gv = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(gd):
        draft(s)
    with torch.cuda.graph(gv):
        verify(s)
    s["ctr"].copy_(_counters(5))
    replayed = iterations(s, gd.replay, gv.replay)
    for a, b in zip(eager, replayed):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert eager[1][4].tolist() == [7, 0, 0, 0]
    assert not torch.equal(eager[0][1], eager[1][1]) or not torch.equal(eager[0][0], eager[1][0])
