"""GPU tests of the per-request sampling kernels (csrc/sample.hip, include/magicdec_hip.h K11 "per request"):
temperature, top_p and top_k read per request from device tensors, greedy requests inside a sampled batch.

The method is bit-equality.  K11 states the per-request filter as the scalar filter on the row whose top-k-dropped
logits are -inf, so for every distinct (T, top_p, top_k) of a batch the scalar entry points (unchanged by this form) run
on a top-k-masked copy of the whole batch, and the per-request kernels must give the requests of that triple the same
tokens and the same statistics, integer for integer.  The mask (`topk_mask`) is a numpy statement -- k-th largest key by
a partition -- that shares nothing with the kernel's radix select; tests/test_sampling_request_cpu.py pins it against
sampling_ref.row_filter.  A direct check against the admissible-outcome oracle of tests/sampling_ref.py, independent of
the scalar kernels, follows, then hand-built top-k edges, invalid device values, both thread counts, a graph replayed
across a set_params(), and the argument checks."""
import numpy as np
import pytest
import torch

from magicdec_amd import ops
from magicdec_amd import sampling_ops as so
from magicdec_amd.Engine.sampling import RequestSampler
from tests import sampling_cases as sc
from tests import sampling_ref as sr
from tests.conftest import parity_report
from tests.test_gpu_sampling import _accept_kernel_equals_cpu, _stats_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
NEG_INF = np.uint16(0xFF80)
GREEDY_KSTAR = 0x10000
VS = [1001, 32000]          # 256-thread form on odd, unaligned rows; the wide() 1024-thread form


# ------------------------------------------------------------------------------------ the top-k reference
def topk_mask(x, k):
    """bf16 tensor [..., V], k -> (copy with every element whose key is below the k-th largest key of its row replaced
    by bf16 -inf, bool array of the survivors).  k <= 0 or k >= V: off."""
    bits = sc.bits_of(x)
    V = bits.shape[-1]
    if not 1 <= k < V:
        return x.clone(), np.ones(bits.shape, dtype=bool)
    key = sr.key16(bits)
    kth = np.partition(key, V - k, axis=-1)[..., V - k:V - k + 1]
    keep = key >= kth
    out = np.where(keep, bits, NEG_INF).astype(np.uint16)
    return torch.from_numpy(out.view(np.int16)).view(BF).reshape(x.shape), keep


def _dev(vals, dtype):
    return torch.tensor(list(vals), dtype=dtype, device=DEV)


def _params(triples):
    T, P, K = zip(*triples)
    return _dev(T, torch.float32), _dev(P, torch.float32), _dev(K, torch.int32)


def _triples(V, B, mix):
    """B (T, top_p, top_k) triples: T x top_p pairs of {0.05, 0.6, 1.0, 4.0} x {0.3, 0.9, 1.0}, top_k through
    {0, 1, 2, 50, V-1, V, V+7}; `mix` rotates the pairing."""
    pairs = [(t, p) for t in (0.05, 0.6, 1.0, 4.0) for p in (0.3, 0.9, 1.0)]
    ks = [0, 1, 2, 50, V - 1, V, V + 7]
    return [(*pairs[(5 * b + 7 * mix) % len(pairs)], ks[(b + 3 * mix) % len(ks)]) for b in range(B)]


def _case(V, B, G, seed, two_token=False, sigma=0.5, it=4):
    """One iteration's inputs in the form of tests/sampling_cases.py; two_token: draft step 0 has two rows per request
    and a row selector."""
    g = torch.Generator().manual_seed(seed)
    tl = (torch.randn(B, G + 1, V, generator=g) * 2.5).to(BF)
    dl = [(tl[:, j:j + 1].float() + torch.randn(B, 1, V, generator=g) * sigma).to(BF) for j in range(G)]
    row_sel = None
    if two_token:
        row_sel = torch.randint(1, 3, (B,), generator=g)
        other = (torch.randn(B, 1, V, generator=g) * 2.5).to(BF)
        dl[0] = torch.cat([torch.where((row_sel == 1).view(B, 1, 1), dl[0], other),
                           torch.where((row_sel == 2).view(B, 1, 1), dl[0], other)], dim=1)
    return dict(name=f"req_v{V}", V=V, B=B, G=G, it=it, seed=sc.SEED + seed, tl=tl, dl=dl, row_sel=row_sel,
                tok0=torch.randint(0, V, (B,), generator=g))


def _buffers(c):
    B, G, V = c["B"], c["G"], c["V"]
    ctr = torch.zeros(4, dtype=torch.int32, device=DEV)
    ctr[0] = c["it"]
    tb = torch.zeros((B, G + 1), dtype=torch.int64, device=DEV)
    tb[:, 0] = c["tok0"].to(DEV)
    return dict(ctr=ctr, tb=tb, ring=torch.zeros((B, G, V), dtype=BF, device=DEV),
                rst=torch.zeros((B, G, 2), dtype=torch.int64, device=DEV),
                tst=torch.zeros((B * (G + 1), 2), dtype=torch.int64, device=DEV))


def _iteration(c, draw, verify, tokens=None):
    """gamma draft launches and the verify of case `c` through draw(x, n, ctr, row_sel, ring, rst) and
    verify(x, tb, ring, rst, tst, ctr); `tokens`: the tokens_buffer the verify reads instead of the drafts just drawn."""
    B, G, V = c["B"], c["G"], c["V"]
    s = _buffers(c)
    sel = c["row_sel"].to(DEV) if c["row_sel"] is not None else None
    for j, x in enumerate(c["dl"]):
        n = x.shape[1]
        t = draw(x.reshape(B * n, V).to(DEV), n, s["ctr"], sel if n == 2 else None, s["ring"], s["rst"])
        assert bool((t == t[:, :1]).all())
        s["tb"][:, j + 1] = t[:, 0]
    assert s["ctr"].tolist() == [c["it"], G, 0, 0]
    drafts = s["tb"][:, 1:].cpu().numpy().copy()
    if tokens is not None:
        s["tb"].copy_(torch.from_numpy(tokens).to(DEV))
    tt = verify(c["tl"].reshape(B * (G + 1), V).to(DEV), s["tb"], s["ring"], s["rst"], s["tst"], s["ctr"])
    torch.cuda.synchronize()
    assert s["ctr"].tolist() == [c["it"] + 1, 0, 0, 0]
    return dict(drafts=drafts, tokens=s["tb"].cpu().numpy(), tt=tt.cpu().numpy(), ring=s["ring"].cpu(),
                rst=_stats_np(s["rst"]), tst=_stats_np(s["tst"]), rst_raw=s["rst"].cpu(), tst_raw=s["tst"].cpu())


def _iter_req(c, triples, top_k=True):
    T, P, K = _params(triples)
    K = K if top_k else None
    seed = c["seed"]
    return _iteration(
        c, lambda x, n, ctr, sel, ring, rst: so.sample_rows_req(x, n, T, P, K, seed, ops.SAMPLE_DRAFT, ctr,
                                                                ops.ADVANCE_STEP, row_sel=sel, ring=ring, ring_stats=rst),
        lambda x, tb, ring, rst, tst, ctr: so.spec_verify_sample_req(x, tb, ring, rst, tst, ctr, T, P, K, seed))


def _iter_scalar(c, T, top_p, tokens):
    seed = c["seed"]
    return _iteration(
        c, lambda x, n, ctr, sel, ring, rst: ops.sample_rows(x, n, T, top_p, seed, ops.SAMPLE_DRAFT, ctr,
                                                             ops.ADVANCE_STEP, row_sel=sel, ring=ring, ring_stats=rst),
        lambda x, tb, ring, rst, tst, ctr: ops.spec_verify_sample(x, tb, ring, rst, tst, ctr, T, top_p, seed),
        tokens=tokens)


def _masked_case(c, k):
    return dict(c, tl=topk_mask(c["tl"], k)[0], dl=[topk_mask(x, k)[0] for x in c["dl"]])


def _same_kept(bits, keep_k, kstar_req, masked_bits, kstar_ref):
    return np.array_equal((sr.key16(bits) >= kstar_req) & keep_k, (sr.key16(masked_bits) >= kstar_ref) & keep_k)


def _equals_scalar(c, o, triples, tag):
    """The sampled requests of per-request outputs `o` against the scalar kernels on masked rows -> requests compared."""
    B, G = c["B"], c["G"]
    drawn = sc.drawn_rows(c)
    assert torch.equal(o["ring"], drawn), f"{tag}: a ring slot is not the unmasked selected row"
    tbits, rbits = sc.bits_of(c["tl"]), sc.bits_of(drawn)
    done = 0
    for T, top_p, k in sorted({t for t in triples if t[0] > 0}):
        who = [b for b in range(B) if triples[b] == (T, top_p, k)]
        mc = _masked_case(c, k)
        ref = _iter_scalar(mc, T, top_p, o["tokens"])
        mt, mr = sc.bits_of(mc["tl"]), sc.bits_of(sc.drawn_rows(mc))
        keep_t, keep_r = topk_mask(c["tl"], k)[1], topk_mask(drawn, k)[1]
        for b in who:
            what = f"{tag}: request {b} (T={T}, top_p={top_p}, top_k={k})"
            assert np.array_equal(o["drafts"][b], ref["drafts"][b]), f"{what}: draft tokens"
            assert np.array_equal(o["tt"][b], ref["tt"][b]), f"{what}: target_tokens"
            for j in range(G):
                i = b * G + j
                assert o["rst"][0][i] == ref["rst"][0][i] and o["rst"][2][i] == ref["rst"][2][i], f"{what}: ring stats {j}"
                assert _same_kept(rbits[b, j], keep_r[b, j], o["rst"][1][i], mr[b, j], ref["rst"][1][i]), f"{what}: ring {j}"
            for j in range(G + 1):
                i = b * (G + 1) + j
                assert o["tst"][0][i] == ref["tst"][0][i] and o["tst"][2][i] == ref["tst"][2][i], f"{what}: target stats {j}"
                assert _same_kept(tbits[b, j], keep_t[b, j], o["tst"][1][i], mt[b, j], ref["tst"][1][i]), f"{what}: target {j}"
            done += 1
    return done


# ------------------------------------------------------------------------------------ 1. bit-equality, mixed batch
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("mix,two_token", [(0, False), (1, True)])
def test_mixed_batch_equals_the_scalar_kernels_on_masked_rows(V, mix, two_token):
    """Draft mode with n = 1 and with the two-token step (n = 2, row_sel), then a verify whose drafts came from the
    per-request draws."""
    B, G = 8, 3
    c = _case(V, B, G, seed=100 + mix, two_token=two_token)
    triples = _triples(V, B, mix)
    o = _iter_req(c, triples)
    assert _equals_scalar(c, o, triples, f"mixed batch V={V} mix={mix}") == B


@pytest.mark.parametrize("V", VS)
def test_prefill_and_baseline_draws_equal_the_scalar_kernels_on_masked_rows(V):
    B, n = 8, 2
    g = torch.Generator().manual_seed(V + 1)
    x = (torch.randn(B * n, V, generator=g) * 2.5).to(BF)
    triples = _triples(V, B, 2)
    T, P, K = _params(triples)
    for purpose in (ops.SAMPLE_PREFILL, ops.SAMPLE_BASELINE):
        ctr = torch.zeros(4, dtype=torch.int32, device=DEV)
        ctr[0] = 6
        tok = so.sample_rows_req(x.to(DEV), n, T, P, K, 77, purpose, ctr, ops.ADVANCE_ITER)
        assert ctr.tolist() == [7, 0, 0, 0] and bool((tok == tok[:, :1]).all())
        for t, p, k in sorted(set(triples)):
            ctr[0] = 6
            ref = ops.sample_rows(topk_mask(x, k)[0].to(DEV), n, t, p, 77, purpose, ctr, ops.ADVANCE_ITER)
            who = [b for b in range(B) if triples[b] == (t, p, k)]
            assert torch.equal(tok[who], ref[who]), (purpose, t, p, k)


# ------------------------------------------------------------------------------------ 2. greedy rows
@pytest.mark.parametrize("V", VS)
def test_greedy_requests_inside_a_sampled_batch(V):
    B, G = 8, 3
    c = _case(V, B, G, seed=7, two_token=True)
    for b in (0, 2):                                    # equal maxima: md_argmax takes the lowest index
        c["tl"][b, :, [V - 1, 3, 7]] = 30.0
        for x in c["dl"]:
            x[b, :, [V - 2, 5, 9]] = 30.0
    triples = [(0.0, 0.9, 50) if b % 2 == 0 else t for b, t in enumerate(_triples(V, B, 1))]
    greedy = [b for b in range(B) if triples[b][0] == 0]
    o = _iter_req(c, triples)
    drawn = sc.drawn_rows(c)
    want_d = ops.argmax(drawn.reshape(B * G, V).to(DEV)).view(B, G).cpu().numpy()
    want_t = ops.argmax(c["tl"].reshape(B * (G + 1), V).to(DEV)).view(B, G + 1).cpu().numpy()
    assert np.array_equal(o["drafts"][greedy], want_d[greedy])
    assert np.array_equal(o["tt"][greedy], want_t[greedy])
    assert (want_d[[0, 2]] == 5).all() and (want_t[[0, 2]] == 3).all()
    assert (o["rst"][1].reshape(B, G)[greedy] == GREEDY_KSTAR).all()        # the documented marker
    assert _equals_scalar(c, o, triples, f"half greedy V={V}") == B - len(greedy)
    # the accept kernel on the per-request target_tokens: for the greedy requests, the greedy loop's own path
    mine = _accept_kernel_equals_cpu(o["tokens"], o["tt"], G, -5, -6)
    loop = _accept_kernel_equals_cpu(o["tokens"], want_t, G, -5, -6)
    for key in ("an", "bonus", "num_nodes", "cachelens", "out"):
        assert torch.equal(mine[key][greedy], loop[key][greedy]), key


# ------------------------------------------------------------------------------------ 3. the direct oracle
def _checked_row(bits, T, top_p, k, m, kstar, zkept, tag):
    """check_stats of the masked row under the request's parameters.  With top-k on and top_p = 1 the kernel stores
    kstar = the k-th largest key (K11) where check_stats expects 0: asserted exactly here, and the two kept sets differ
    only by -inf entries of probability 0."""
    masked, _ = topk_mask(torch.from_numpy(bits.view(np.int16).copy()).view(BF), k)
    mb = sc.bits_of(masked)
    if top_p >= 1 and 1 <= k < len(bits):
        assert int(kstar) == int(np.sort(sr.key16(bits))[len(bits) - k]), f"{tag}: kstar {int(kstar):#x}"
        kstar = 0
    return sr.check_stats(mb, T, top_p, m, kstar, zkept, tag=tag)


@pytest.mark.parametrize("V", VS)
def test_mixed_batch_lies_in_the_admissible_set_of_the_restatement(V):
    B, G = 8, 3
    c = _case(V, B, G, seed=300)
    triples = _triples(V, B, 0)
    o = _iter_req(c, triples)
    tbits, rbits = sc.bits_of(c["tl"]), sc.bits_of(sc.drawn_rows(c))
    ambiguous = 0
    for b, (T, top_p, k) in enumerate(triples):
        rrows = [_checked_row(rbits[b, j], T, top_p, k, *(a[b * G + j] for a in o["rst"]), tag=f"ring[{b},{j}]")
                 for j in range(G)]
        trows = [_checked_row(tbits[b, j], T, top_p, k, *(a[b * (G + 1) + j] for a in o["tst"]), tag=f"target[{b},{j}]")
                 for j in range(G + 1)]
        multi = False
        for j in range(G):
            adm = sr.draw_admissible(rrows[j], c["seed"], sr.DRAFT, j, b, c["it"])
            assert o["drafts"][b, j] in adm, (b, j, o["drafts"][b, j], adm.tolist())
            multi |= len(adm) > 1
        outs = sr.verify_admissible(trows, rrows, o["tokens"][b], c["seed"], b, c["it"])
        assert sr.contains(outs, o["tt"][b]), (b, o["tt"][b].tolist(), [x.tolist() for x in outs[:8]])
        ambiguous += bool(multi or len(outs) > 1)
    parity_report(f"[sampling] per-request mixed batch V={V} B={B} gamma={G}: stats of {B * (2 * G + 1)} masked rows "
                  f"checked, {B} requests restated with their own (T, top_p, top_k), {ambiguous} with more than one "
                  f"admissible outcome, 0 tokens outside the admissible set")


# ------------------------------------------------------------------------------------ 4. top-k edges
def _edge(row, T, top_p, k, N=2048, it=6, seed=321):
    """One hand-built row for N requests (row stride 0) in draft mode, per-request against scalar-on-masked ->
    (tokens [N], kstar, zkept of request 0)."""
    xb = torch.as_tensor(row, dtype=torch.float32).to(BF).view(1, -1)
    V = xb.shape[1]

    def run(x, draw):
        ctr = torch.zeros(4, dtype=torch.int32, device=DEV)
        ctr[0] = it
        ring = torch.zeros((N, 1, V), dtype=BF, device=DEV)
        rst = torch.zeros((N, 1, 2), dtype=torch.int64, device=DEV)
        tok = draw(x.to(DEV).expand(N, V), ctr, ring, rst)
        torch.cuda.synchronize()
        return tok[:, 0].cpu().numpy(), _stats_np(rst), ring
    T_, P_, K_ = _params([(T, top_p, k)] * N)
    tok, st, ring = run(xb, lambda x, ctr, ring, rst: so.sample_rows_req(
        x, 1, T_, P_, K_, seed, ops.SAMPLE_DRAFT, ctr, ops.ADVANCE_STEP, ring=ring, ring_stats=rst))
    masked, keep = topk_mask(xb, k)
    rtok, rs, _ = run(masked, lambda x, ctr, ring, rst: ops.sample_rows(
        x, 1, T, top_p, seed, ops.SAMPLE_DRAFT, ctr, ops.ADVANCE_STEP, ring=ring, ring_stats=rst))
    assert np.array_equal(tok, rtok)
    assert np.array_equal(st[0], rs[0]) and np.array_equal(st[2], rs[2])
    assert (st[1] == st[1][0]).all() and (rs[1] == rs[1][0]).all()
    assert _same_kept(sc.bits_of(xb)[0], keep[0], st[1][0], sc.bits_of(masked)[0], rs[1][0])
    assert torch.equal(ring[:, 0].cpu(), xb.expand(N, V))
    return tok, int(st[1][0]), int(st[2][0])


def _key(v):
    return int(sr.key16(sr.bf16_bits(np.float32(v))))


def test_top_k_keeps_a_tie_group_across_place_k_whole():
    row = [3.0] + [2.0] * 4 + [1.0] * 3 + [0.0] * 20
    tok, kstar, zk = _edge(row, 1.0, 1.0, 3)                    # place 3 is inside the group of four 2.0
    assert kstar == _key(2.0)
    counts = np.bincount(tok, minlength=len(row))
    assert counts[5:].sum() == 0 and (counts[:5] > 0).all()
    tok, kstar, zk = _edge(row, 1.0, 1.0, 5)                    # the group ends at place 5: nothing more is kept
    assert kstar == _key(2.0) and np.bincount(tok, minlength=len(row))[5:].sum() == 0


def test_top_k_one_returns_a_member_of_the_maximal_tie_group():
    V = 1001
    g = torch.Generator().manual_seed(2)
    row = torch.randn(V, generator=g)
    row[[900, 17, 5]] = 6.0
    tok, kstar, zk = _edge(row, 0.7, 0.9, 1)
    assert set(tok.tolist()) == {5, 17, 900} and zk == 3 * 2 ** 40 and kstar == _key(6.0)
    row[5] = 6.5
    tok, kstar, zk = _edge(row, 0.7, 0.9, 1)
    assert (tok == 5).all() and zk == 2 ** 40
    # without noise (T = 0) the equal scores resolve to the lowest index, md_argmax's rule
    row[5] = 6.0
    xb = row.to(BF).view(1, V).to(DEV)
    T_, P_, K_ = _params([(0.0, 0.9, 1)])
    ctr = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert so.sample_rows_req(xb, 1, T_, P_, K_, 1, ops.SAMPLE_BASELINE, ctr, ops.ADVANCE_ITER).tolist() == [[5]]
    assert ops.argmax(xb).tolist() == [5]


def test_top_k_and_top_p_boundaries_in_the_same_and_in_different_bins():
    """The high byte of a key is the sign and seven exponent bits: powers of two sit in different bins, [1, 2) in one."""
    spread = [8.0, 4.0, 2.0, 1.0, 0.5, 0.25, 0.125] + [-3.0] * 30
    # top-p tighter than top-k, in another bin: 8.0 carries 0.96 of the top-5 mass
    tok, kstar, zk = _edge(spread, 1.0, 0.6, 5)
    assert kstar == _key(8.0) and (tok == 0).all() and zk == 2 ** 40
    # top-k tighter than top-p: top_p = 0.999 would keep more than the 5 survivors
    tok, kstar, zk = _edge(spread, 4.0, 0.999, 5)
    assert kstar == _key(0.5) and set(tok.tolist()) == {0, 1, 2, 3, 4}
    # top-p boundary two bins above the k-th key: masses 1, .368, .223, .174, .153 -> 2.0 is kept (1.368 <= 0.75 Z =
    # 1.438), 1.0 is not (1.591)
    tok, kstar, zk = _edge(spread, 4.0, 0.75, 5)
    assert kstar == _key(2.0) and set(tok.tolist()) == {0, 1, 2}
    # both boundaries inside one bin: the low-byte masses of the top-k pass serve the top-p select
    dense = [1.0 + i / 16 for i in range(16)] + [0.25] * 30
    tok, kstar, zk = _edge(dense, 0.05, 0.9, 8)                 # masses 1, .287, .082, ...: Z = 1.401, 1 <= 0.9 Z < 1.287
    assert kstar == _key(1.875) and set(tok.tolist()) == {14, 15}
    tok, kstar, zk = _edge(dense, 4.0, 0.5, 8)                  # masses e^(-j/64): Z = 7.58, four tokens above the cut
    assert kstar == _key(1.75) and set(tok.tolist()) == {12, 13, 14, 15}
    tok, kstar, zk = _edge(dense, 4.0, 1.0, 8)
    assert kstar == _key(1.0 + 8 / 16) and set(tok.tolist()) == set(range(8, 16))


def test_top_k_with_minus_infinity_entries_and_k_beyond_the_finite_ones():
    row = [float("-inf")] * 40
    for i, v in ((3, 1.0), (11, 0.5), (12, 0.5), (29, -1.0), (39, 2.0)):
        row[i] = v
    for top_p in (1.0, 0.95):
        tok, kstar, zk = _edge(row, 1.0, top_p, 10)             # ten places, five finite logits: all five survive
        assert set(tok.tolist()) <= {3, 11, 12, 29, 39} and len(set(tok.tolist())) >= 4
    tok, kstar, zk = _edge(row, 1.0, 1.0, 10)
    assert kstar == _key(float("-inf"))
    tok, kstar, zk = _edge(row, 1.0, 1.0, 3)                    # place 3 is inside the pair of 0.5
    assert kstar == _key(0.5) and set(tok.tolist()) == {3, 11, 12, 39}


def test_top_k_signed_zeros_at_the_boundary():
    row = [1.0, 0.0, -0.0, -0.0] + [-5.0] * 20
    tok, kstar, zk = _edge(row, 1.0, 1.0, 2)                    # +0 is place 2; -0 has the smaller key
    assert kstar == 0x8000 and set(tok.tolist()) == {0, 1}
    tok, kstar, zk = _edge(row, 1.0, 1.0, 3)                    # place 3 is inside the pair of -0
    assert kstar == 0x7FFF and set(tok.tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("V", VS)
def test_top_k_at_extreme_temperatures(V):
    g = torch.Generator().manual_seed(V)
    row = torch.randn(V, generator=g) * 2.5
    n = int(topk_mask(row.to(BF), 50)[1].sum())                 # 50, plus the rest of a tie group at place 50
    assert 50 <= n < 80
    tok, kstar, zk = _edge(row, 0.05, 0.9, 50, N=256)           # most masses are zero
    assert 2 ** 40 <= zk < n * 2 ** 40 // 4
    # all masses near 2^40 (l - m > -25, so each is above e^-0.5 2^40); the kept mass exceeds top_p Z_k
    tok, kstar, zk = _edge(row, 50.0, 0.9, 50, N=256)
    assert 0.9 * 0.6 * n * 2 ** 40 < zk <= n * 2 ** 40


# ------------------------------------------------------------------------------------ 5. invalid device values
@pytest.mark.parametrize("V", VS)
def test_invalid_device_values_take_their_documented_meaning(V):
    B, G = 8, 3
    c = _case(V, B, G, seed=500)
    nan = float("nan")
    bad = [(nan, 0.9, 50), (-1.0, 0.9, 0), (0.6, 0.0, 50), (0.6, -1.0, 0), (1.0, 2.0, 2), (1.0, nan, 50),
           (0.6, 0.9, -3), (4.0, nan, -(2 ** 31))]
    good = [(0.0, 0.9, 50), (0.0, 0.9, 0), (0.6, 1.0, 50), (0.6, 1.0, 0), (1.0, 1.0, 2), (1.0, 1.0, 50),
            (0.6, 0.9, 0), (4.0, 1.0, 0)]
    a, b = _iter_req(c, bad), _iter_req(c, good)
    assert np.array_equal(a["drafts"], b["drafts"]) and np.array_equal(a["tt"], b["tt"])
    assert torch.equal(a["rst_raw"], b["rst_raw"]) and torch.equal(a["tst_raw"], b["tst_raw"])
    assert torch.equal(a["ring"], b["ring"])
    # top_k = NULL is top-k off for every request
    off = [(t, p, 0) for t, p, _ in good]
    a, b = _iter_req(c, off, top_k=False), _iter_req(c, off)
    assert np.array_equal(a["drafts"], b["drafts"]) and np.array_equal(a["tt"], b["tt"])
    assert torch.equal(a["rst_raw"], b["rst_raw"]) and torch.equal(a["tst_raw"], b["tst_raw"])


# ------------------------------------------------------------------------------------ 6. thread counts
def test_per_request_results_do_not_depend_on_the_thread_count():
    """As test_gpu_sampling.py::test_results_do_not_depend_on_the_thread_count: the same rows at the same request
    indices in a batch of 8 (every kernel on 1024 threads) and in a batch of 520 (every kernel on 256 threads)."""
    big, small = sc.thread_count_cases()
    G, Bs, V = small["G"], small["B"], small["V"]
    head = [(0.6, 0.9, 50), (0.0, 1.0, 0), (1.0, 1.0, 2), (4.0, 0.3, V - 1), (0.05, 0.9, 0), (1.0, 0.3, 1),
            (0.6, 1.0, 700), (0.0, 0.9, 50)]
    tail = [head[b % len(head)] for b in range(Bs, big["B"])]
    ob, os_ = _iter_req(big, head + tail), _iter_req(small, head)
    assert torch.equal(ob["rst_raw"][:Bs], os_["rst_raw"]) and torch.equal(ob["tst_raw"][:Bs * (G + 1)], os_["tst_raw"])
    assert np.array_equal(ob["drafts"][:Bs], os_["drafts"]) and np.array_equal(ob["tt"][:Bs], os_["tt"])
    assert torch.equal(ob["ring"][:Bs], os_["ring"])
    assert _equals_scalar(small, os_, head, "thread count (1024 threads)") == 6


# ------------------------------------------------------------------------------------ 7. graph capture
def test_graph_replays_follow_set_params_without_a_recapture():
    V, B, G, K, seed = 32000, 4, 2, 4, 4242
    g = torch.Generator().manual_seed(12)
    tls = [(torch.randn(B * (G + 1), V, generator=g) * 2.5).to(BF) for _ in range(K)]
    dls = [[(tls[k].view(B, G + 1, V)[:, j].float() + torch.randn(B, V, generator=g) * 0.5).to(BF) for j in range(G)]
           for k in range(K)]
    first = ([0.8, 0.0, 1.0, 0.6], [0.9, 1.0, 0.3, 1.0], [0, 0, 50, 2])
    second = ([0.0, 1.5, 0.6, 0.0], 0.9, [3, 700, 0, 0])
    schedule = [first, first, second, second]

    def state():
        return dict(smp=RequestSampler(*first, seed, B, G, V, DEV),
                    tb=torch.full((B, G + 1), 3, dtype=torch.int64, device=DEV),
                    tt=torch.zeros((B, G + 1), dtype=torch.int64, device=DEV))

    def iteration(s, dx, tx):
        for j in range(G):
            s["tb"][:, j + 1].copy_(s["smp"].head(dx[j], "draft", None, B, 1)[:, 0])
        s["tt"].copy_(s["smp"].head(tx, "verify", s["tb"], B, G + 1))

    s = state()
    dx = [dls[0][j].to(DEV) for j in range(G)]
    tx = tls[0].to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        iteration(s, dx, tx)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    s["smp"].reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        iteration(s, dx, tx)
    s["smp"].captured = True                            # what Engine/graph.py sets: set_params must still be allowed
    seen = set()
    for k in range(K):
        for j in range(G):
            dx[j].copy_(dls[k][j])
        tx.copy_(tls[k])
        s["smp"].set_params(*schedule[k])
        graph.replay()
        torch.cuda.synchronize()
        e = state()
        e["smp"].counters[0] = k
        e["smp"].set_params(*schedule[k])
        iteration(e, [x.to(DEV) for x in dls[k]], tls[k].to(DEV))
        torch.cuda.synchronize()
        for key in ("tt", "tb"):
            assert torch.equal(s[key], e[key]), (k, key)
        for key in ("ring", "ring_stats", "target_stats"):
            assert torch.equal(getattr(s["smp"], key), getattr(e["smp"], key)), (k, key)
        assert s["smp"].counters.tolist() == [k + 1, 0, 0, 0] == e["smp"].counters.tolist()
        seen.add(tuple(s["tt"].flatten().tolist()))
    assert len(seen) == K


# ------------------------------------------------------------------------------------ 8. bad arguments
def test_per_request_wrappers_reject_bad_parameter_tensors():
    B, G, V = 4, 2, 64
    x = torch.zeros((B, V), dtype=BF, device=DEV)
    xv = torch.zeros((B * (G + 1), V), dtype=BF, device=DEV)
    ctr = torch.zeros(4, dtype=torch.int32, device=DEV)
    ring = torch.zeros((B, G, V), dtype=BF, device=DEV)
    rst = torch.zeros((B, G, 2), dtype=torch.int64, device=DEV)
    tst = torch.zeros((B * (G + 1), 2), dtype=torch.int64, device=DEV)
    tb = torch.zeros((B, G + 1), dtype=torch.int64, device=DEV)
    T, P, K = _params([(1.0, 0.9, 5)] * B)

    def draw(T=T, P=P, K=K, logits=x):
        return so.sample_rows_req(logits, 1, T, P, K, 1, ops.SAMPLE_DRAFT, ctr, ops.ADVANCE_STEP, ring=ring,
                                  ring_stats=rst)

    def verify(T=T, P=P, K=K, logits=xv):
        return so.spec_verify_sample_req(logits, tb, ring, rst, tst, ctr, T, P, K, 1)

    bad = []
    for f in (draw, verify):
        bad += [lambda f=f: f(T=T.double()), lambda f=f: f(T=T.to(BF)), lambda f=f: f(P=P.half()),
                lambda f=f: f(K=K.long()), lambda f=f: f(K=K.float()),                      # dtypes
                lambda f=f: f(T=T[:B - 1]), lambda f=f: f(P=P.view(B, 1)), lambda f=f: f(K=K[:1]),
                lambda f=f: f(T=T.repeat(2)), lambda f=f: f(T=T.repeat(2)[::2]),           # shapes, strides
                lambda f=f: f(T=T.cpu()), lambda f=f: f(P=P.cpu()), lambda f=f: f(K=K.cpu()),
                lambda f=f: f(T=None), lambda f=f: f(P=None), lambda f=f: f(T=1.0), lambda f=f: f(P=0.9),
                lambda f=f: f(logits=x.float())]
    for i, f in enumerate(bad):
        with pytest.raises((ValueError, TypeError, ops.MagicDecHipError)):
            f()
            pytest.fail(f"bad call {i} was accepted")
    torch.cuda.synchronize()
    assert ctr.tolist() == [0, 0, 0, 0]                  # nothing was launched
    draw()
    verify(K=None)
    torch.cuda.synchronize()
    assert ctr.tolist() == [1, 0, 0, 0]
