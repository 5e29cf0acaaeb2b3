"""GPU tests of the sampling kernels (csrc/sample.hip, include/magicdec_hip.h K11) through the C ABI: the row sampler
against the numpy restatement (tests/sampling_ref.py), determinism and graph replays, the drawn distribution, the
lossless speculative verify, and the verify kernel followed by the unchanged accept kernel.

Second half: whole draft / verify iterations against the admissible-outcome oracle of tests/sampling_ref.py (the
kernel's own row statistics are checked first, then every token must be one the kernel's fp32 arithmetic can reach) --
at the real vocabularies in both the 256- and the 1024-thread instantiation of all three kernels, and at the edges:
odd vocabularies, unaligned and strided rows, -inf entries, tie groups, signed zeros, tiny top_p, extreme temperatures,
out-of-range draft tokens, the zero-residual fallback, end-of-text drafts, graph replays, argument validation.  Rows
made entirely of NaN, +inf or -inf are out of scope: K11 does not define them.
The inputs of the real-vocabulary cases live in tests/sampling_cases.py, where the CPU suite checks that they leave
(almost) no request ambiguous."""
import numpy as np
import pytest
import torch

from magicdec_amd import ops
from tests import sampling_cases as sc
from tests import sampling_ref as sr
from tests.conftest import parity_report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHI2_LEVEL = 1e-6


def _counters():
    return torch.zeros(4, dtype=torch.int32, device=DEV)


def _stats_np(st):
    """[..., 2] int64 md_sample_stats -> (m float32, kstar uint32, zkept uint64) arrays."""
    a = st.cpu().numpy().reshape(-1, 2)
    lo = a[:, 0].astype(np.int64).view(np.uint64)
    m = (lo & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)
    kstar = (lo >> np.uint64(32)).astype(np.uint32)
    return m, kstar, a[:, 1].view(np.uint64)


def _chi2_ok(counts, probs):
    keep = probs > 0
    assert counts[~keep].sum() == 0, "a token outside the support was drawn"
    n = counts.sum()
    exp = probs[keep] * n
    chi2 = float(((counts[keep] - exp) ** 2 / exp).sum())
    dof = max(int(keep.sum()) - 1, 1)
    # chi-square survival function = regularised upper incomplete gamma Q(dof / 2, chi2 / 2)
    pval = float(torch.special.gammaincc(torch.tensor(dof / 2, dtype=torch.float64),
                                         torch.tensor(chi2 / 2, dtype=torch.float64)))
    return pval > CHI2_LEVEL, pval


@pytest.mark.parametrize("V", [1000, 32000, 128256, 151936])
@pytest.mark.parametrize("top_p", [0.9, 1.0])
def test_row_sampler_matches_the_restatement(V, top_p):
    T, seed, it = 0.6, 0x1234_5678_9ABC, 5
    B = 16
    g = torch.Generator().manual_seed(V)
    logits = (torch.randn(B, V, generator=g) * 3).to(torch.bfloat16)
    logits[3, 7] = logits[3].max() + 1                  # a peaked row
    logits[5, : V // 2] = logits[5, 0]                  # a big tie group
    x = logits.to(DEV)
    ctr = _counters()
    ctr[0] = it
    ring = torch.zeros((B, 1, V), dtype=torch.bfloat16, device=DEV)
    rst = torch.zeros((B, 1, 2), dtype=torch.int64, device=DEV)
    tok = ops.sample_rows(x, 1, T, top_p, seed, ops.SAMPLE_DRAFT, ctr, ops.ADVANCE_STEP, ring=ring, ring_stats=rst)
    torch.cuda.synchronize()
    assert torch.equal(ring[:, 0], x)                  # the ring row is the input row
    assert ctr.tolist() == [it, 1, 0, 0]
    m, kstar, zk = _stats_np(rst)
    bits = logits.view(torch.int16).numpy().view(np.uint16)
    flagged = diff = 0
    for b in range(B):
        ref_tok, f, fl = sr.draw(bits[b], T, top_p, seed, sr.DRAFT, 0, b, it)
        assert m[b] == np.float32(f["m"])
        if f["margin"] >= sr.TOL:
            assert kstar[b] == f["kstar"], (b, kstar[b], f["kstar"])
            assert abs(float(zk[b]) / 2.0 ** 40 - f["zkept"]) <= 1e-5 * f["zkept"], (b, zk[b], f["zkept"])
        flagged += fl
        if int(tok[b, 0]) != ref_tok:
            diff += 1
            assert fl, (b, int(tok[b, 0]), ref_tok)
    parity_report(f"[sampling] row sampler V={V} top_p={top_p}: {B} rows, {flagged} flagged near-ties, "
                  f"{diff} token differences (all at flagged rows)")


def test_two_launches_are_bit_identical_and_graph_replays_advance_the_stream():
    V, B, T, top_p, seed = 32000, 8, 1.0, 0.95, 99
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(B * 2, V, generator=g) * 2).to(torch.bfloat16).to(DEV)
    sel = torch.tensor([1, 2] * (B // 2), dtype=torch.int64, device=DEV)
    outs = []
    for _ in range(2):
        ctr = _counters()
        ring = torch.zeros((B, 3, V), dtype=torch.bfloat16, device=DEV)
        rst = torch.zeros((B, 3, 2), dtype=torch.int64, device=DEV)
        t0 = ops.sample_rows(x, 2, T, top_p, seed, ops.SAMPLE_DRAFT, ctr, ops.ADVANCE_STEP, row_sel=sel, ring=ring,
                             ring_stats=rst)
        t1 = ops.sample_rows(x, 2, T, top_p, seed, ops.SAMPLE_DRAFT, ctr, ops.ADVANCE_STEP, row_sel=sel, ring=ring,
                             ring_stats=rst)
        torch.cuda.synchronize()
        outs.append((t0.clone(), t1.clone(), ring.clone(), rst.clone(), ctr.clone()))
        # the selected row of each request went to the ring (slots 0 and 1), the token is in both columns
        rows = x.view(B, 2, V)[torch.arange(B), sel.cpu() - 1]
        assert torch.equal(ring[:, 0], rows) and torch.equal(ring[:, 1], rows)
        assert torch.equal(t0[:, 0], t0[:, 1])
        assert ctr.tolist() == [0, 2, 0, 0]
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    # the eager stats equal the stored ones
    assert torch.equal(outs[0][3][:, 0], outs[0][3][:, 1])

    # graph: the counters are read on the device, so successive replays draw differently and advance the iteration
    ctr = _counters()
    out = torch.zeros((B, 1), dtype=torch.int64, device=DEV)
    xr = x[:B].contiguous()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.sample_rows(xr, 1, T, top_p, seed, ops.SAMPLE_BASELINE, ctr, ops.ADVANCE_ITER, out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    ctr.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.sample_rows(xr, 1, T, top_p, seed, ops.SAMPLE_BASELINE, ctr, ops.ADVANCE_ITER, out=out)
    draws = []
    for _ in range(4):
        graph.replay()
        torch.cuda.synchronize()
        draws.append(out[:, 0].clone())
    assert ctr.tolist() == [4, 0, 0, 0]
    assert len({tuple(d.tolist()) for d in draws}) == 4
    # replay k equals an eager launch at iteration k
    ctr2 = _counters()
    ctr2[0] = 2
    eager = ops.sample_rows(xr, 1, T, top_p, seed, ops.SAMPLE_BASELINE, ctr2, ops.ADVANCE_ITER)
    assert torch.equal(eager[:, 0], draws[2])


@pytest.mark.parametrize("T,top_p", [(1.0, 1.0), (0.7, 0.8)])
def test_drawn_distribution_passes_chi_square(T, top_p):
    V, N = 50, 1 << 18
    g = torch.Generator().manual_seed(7)
    row = (torch.randn(V, generator=g) * 1.5).to(torch.bfloat16)
    x = row.to(DEV).view(1, V).expand(N, V)            # one row, N requests (row stride 0)
    tok = ops.sample_rows(x, 1, T, top_p, 2024, ops.SAMPLE_BASELINE, _counters(), ops.ADVANCE_ITER)
    counts = np.bincount(tok[:, 0].cpu().numpy(), minlength=V)
    p = sr.probs(sr.row_filter(row.view(torch.int16).numpy().view(np.uint16), T, top_p))
    ok, pval = _chi2_ok(counts, p)
    assert ok, pval


def _verify_case(p_logits, q_logits, T, top_p, N, seed=77):
    """p_logits [G+1, V], q_logits [G, V] (float32, -inf allowed): drafts drawn by the row sampler (ring slots j),
    then the verify kernel.  -> (tokens_buffer, target_tokens) on the host."""
    G1, V = p_logits.shape
    G = G1 - 1
    pb = p_logits.to(torch.bfloat16).to(DEV)
    qb = q_logits.to(torch.bfloat16).to(DEV)
    ctr = _counters()
    ring = torch.zeros((N, G, V), dtype=torch.bfloat16, device=DEV)
    rst = torch.zeros((N, G, 2), dtype=torch.int64, device=DEV)
    tb = torch.zeros((N, G1), dtype=torch.int64, device=DEV)
    for j in range(G):
        t = ops.sample_rows(qb[j].view(1, V).expand(N, V), 1, T, top_p, seed, ops.SAMPLE_DRAFT, ctr, ops.ADVANCE_STEP,
                            ring=ring, ring_stats=rst)
        tb[:, j + 1] = t[:, 0]
    logits = pb.view(1, G1, V).expand(N, G1, V).reshape(N * G1, V).contiguous()
    tst = torch.zeros((N * G1, 2), dtype=torch.int64, device=DEV)
    tt = ops.spec_verify_sample(logits, tb, ring, rst, tst, ctr, T, top_p, seed)
    torch.cuda.synchronize()
    assert ctr.tolist() == [1, 0, 0, 0]
    return tb.cpu().numpy(), tt.cpu().numpy()


def _filtered(logits_row, T, top_p):
    bits = logits_row.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    return sr.probs(sr.row_filter(bits, T, top_p))


@pytest.mark.parametrize("case", ["q_equals_p", "shifted", "peaked_elsewhere", "disjoint"])
def test_speculative_verify_is_lossless(case):
    V, G, N, T, top_p = 50, 3, 1 << 18, 1.0, 0.95
    g = torch.Generator().manual_seed(11)
    p = torch.randn(G + 1, V, generator=g) * 1.2
    if case == "q_equals_p":
        q = p[:G].clone()
    elif case == "shifted":
        q = p[:G] + torch.randn(G, V, generator=g) * 0.8
    elif case == "peaked_elsewhere":
        q = p[:G].clone()
        q[:, 3] = p[:G].max() + 3.0
    else:
        p[:, V // 2:] = float("-inf")
        q = torch.randn(G, V, generator=g)
        q[:, : V // 2] = float("-inf")
    tb, tt = _verify_case(p, q, T, top_p, N)
    acc = np.zeros(N, dtype=np.int64)
    alive = np.ones(N, dtype=bool)
    for j in range(G):
        alive &= tt[:, j] == tb[:, j + 1]
        acc += alive
    pt = [_filtered(p[j], T, top_p) for j in range(G + 1)]
    qt = [_filtered(q[j], T, top_p) for j in range(G)]
    # the first emitted token follows p~_0
    ok, pval = _chi2_ok(np.bincount(tt[:, 0], minlength=V), pt[0])
    assert ok, ("first token", pval)
    if case == "q_equals_p":
        assert (acc == G).all()
        ok, pval = _chi2_ok(np.bincount(tt[:, G], minlength=V), pt[G])
        assert ok, ("bonus", pval)
        return
    beta = [float(np.minimum(pt[j], qt[j]).sum()) for j in range(G)]
    ge = [float(np.prod(beta[:k])) for k in range(G + 2)]
    pk = np.array([ge[k] - (ge[k + 1] if k < G else 0.0) for k in range(G + 1)])
    hist = np.bincount(acc, minlength=G + 1)
    if case == "disjoint":
        assert (acc == 0).all()
    else:
        ok, pval = _chi2_ok(hist, pk)
        assert ok, ("accept counts", hist.tolist(), pk.tolist(), pval)
    # the corrected token is never the rejected draft
    rej = acc < G
    assert not np.any(tt[rej, acc[rej]] == tb[rej, acc[rej] + 1])


def test_verify_then_accept_kernel_leaves_the_predicted_state():
    from tests import cpu_ops
    V, G, B, T, top_p, seed = 1000, 3, 48, 0.8, 0.9, 31337
    g = torch.Generator().manual_seed(5)
    tl = (torch.randn(B, G + 1, V, generator=g) * 2.5).to(torch.bfloat16)
    dl = (tl[:, :G].float() + torch.randn(B, G, V, generator=g)).to(torch.bfloat16)
    ctr = _counters()
    ctr[0] = 3
    ring = torch.zeros((B, G, V), dtype=torch.bfloat16, device=DEV)
    rst = torch.zeros((B, G, 2), dtype=torch.int64, device=DEV)
    tb = torch.zeros((B, G + 1), dtype=torch.int64, device=DEV)
    tb[:, 0] = torch.randint(0, V, (B,), generator=g).to(DEV)
    for j in range(G):
        tb[:, j + 1] = ops.sample_rows(dl[:, j].contiguous().to(DEV), 1, T, top_p, seed, ops.SAMPLE_DRAFT, ctr,
                                       ops.ADVANCE_STEP, ring=ring, ring_stats=rst)[:, 0]
    tst = torch.zeros((B * (G + 1), 2), dtype=torch.int64, device=DEV)
    tt = ops.spec_verify_sample(tl.view(B * (G + 1), V).to(DEV), tb, ring, rst, tst, ctr, T, top_p, seed)
    torch.cuda.synchronize()
    tbits = tl.view(torch.int16).numpy().view(np.uint16)
    dbits = dl.view(torch.int16).numpy().view(np.uint16)
    tbh = tb.cpu().numpy()
    flagged = 0
    for b in range(B):
        for j in range(G):
            ref, _, fl = sr.draw(dbits[b, j], T, top_p, seed, sr.DRAFT, j, b, 3)
            assert ref == tbh[b, j + 1] or fl
        ref_tt, fl = sr.verify(tbits[b], dbits[b], tbh[b], T, top_p, seed, b, 3)
        if not np.array_equal(ref_tt, tt[b].cpu().numpy()):
            assert fl, (b, ref_tt, tt[b].tolist())
            flagged += 1
    parity_report(f"[sampling] verify vs restatement: {B} requests, {flagged} target_tokens rows differ (all flagged)")

    def state():
        return dict(out=torch.zeros((B, 64), dtype=torch.long), num_nodes=torch.full((B,), 20, dtype=torch.long),
                    cachelens=torch.full((B,), 20 + G + 1, dtype=torch.int32),
                    lpl=torch.full((B,), 20 + G + 1, dtype=torch.int32), an=torch.zeros(B, dtype=torch.long),
                    bonus=torch.zeros(B, dtype=torch.long), dbl=torch.zeros((B, 2), dtype=torch.long),
                    cu=torch.ones(B, dtype=torch.long), flags=torch.zeros(2, dtype=torch.int32))
    h, d = state(), {k: v.to(DEV) for k, v in state().items()}
    tbc = tb.cpu().clone()
    cpu_ops.accept_rollback(tbc, tt.cpu(), h["out"], h["num_nodes"], h["cachelens"], h["lpl"], None, None, G, G, G,
                            -5, -6, 10 ** 6, h["an"], h["bonus"], h["dbl"], h["cu"], h["flags"])
    ops.accept_rollback(tb, tt, d["out"], d["num_nodes"], d["cachelens"], d["lpl"], None, None, G, G, G, -5, -6,
                        10 ** 6, d["an"], d["bonus"], d["dbl"], d["cu"], d["flags"])
    torch.cuda.synchronize()
    for k in h:
        assert torch.equal(h[k], d[k].cpu()), k
    assert torch.equal(tbc, tb.cpu())


# ------------------------------------------------------------------------------------ whole iterations vs the oracle
def _dev_rows(x2d, pad):
    """[rows, V] bf16 on the host -> the same rows on the device, dense or (pad = (offset, extra)) as a column slice of
    a wider tensor whose other columns hold a large logit (reading one of them would change every statistic)."""
    if pad is None:
        return x2d.contiguous().to(DEV)
    off, extra = pad
    rows, V = x2d.shape
    full = torch.full((rows, off + V + extra), 60.0, dtype=torch.bfloat16, device=DEV)
    full[:, off:off + V] = x2d.to(DEV)
    return full[:, off:off + V]


def _run_iteration(c, tokens_edit=None, ring_stats_edit=None):
    """gamma draft launches (ring slots 0..gamma-1) and the verify of case `c` (tests/sampling_cases.py) -> host
    arrays dict(ring, rst, tst, drafts, tokens, tt, ctr).  tokens_edit(tb) / ring_stats_edit(rst) change what the verify
    reads after the draft launches."""
    V, B, G, T, top_p, seed = c["V"], c["B"], c["G"], c["T"], c["top_p"], c["seed"]
    ctr = _counters()
    ctr[0] = c["it"]
    ring = torch.zeros((B, G, V), dtype=torch.bfloat16, device=DEV)
    rst = torch.zeros((B, G, 2), dtype=torch.int64, device=DEV)
    tst = torch.zeros((B * (G + 1), 2), dtype=torch.int64, device=DEV)
    tb = torch.zeros((B, G + 1), dtype=torch.int64, device=DEV)
    tb[:, 0] = c["tok0"].to(DEV)
    sel = c["row_sel"].to(DEV) if c["row_sel"] is not None else None
    for j, x in enumerate(c["dl"]):
        n = x.shape[1]
        t = ops.sample_rows(_dev_rows(x.reshape(B * n, V), c["pad"]), n, T, top_p, seed, ops.SAMPLE_DRAFT, ctr,
                            ops.ADVANCE_STEP, row_sel=sel if n == 2 else None, ring=ring, ring_stats=rst)
        assert bool((t == t[:, :1]).all())              # the token goes to every column
        tb[:, j + 1] = t[:, 0]
    assert ctr.tolist() == [c["it"], G, 0, 0]
    drafts = tb[:, 1:].cpu().numpy().copy()
    if tokens_edit is not None:
        tokens_edit(tb)
    if ring_stats_edit is not None:
        ring_stats_edit(rst)
    tt = ops.spec_verify_sample(_dev_rows(c["tl"].reshape(B * (G + 1), V), c["pad"]), tb, ring, rst, tst, ctr, T, top_p,
                                seed)
    torch.cuda.synchronize()
    return dict(ring=sc.bits_of(ring.cpu()), rst=_stats_np(rst), tst=_stats_np(tst), drafts=drafts,
                tokens=tb.cpu().numpy(), tt=tt.cpu().numpy(), ctr=ctr.tolist(), rst_raw=rst.cpu(), tst_raw=tst.cpu())


def _check(c, o, what):
    assert o["ctr"] == [c["it"] + 1, 0, 0, 0]
    n, amb = sc.check_iteration(c, o["ring"], o["rst"], o["tst"], o["drafts"], o["tt"], o["tokens"])
    rows = c["B"] * (2 * c["G"] + 1)
    parity_report(f"[sampling] {what} V={c['V']} B={c['B']} gamma={c['G']} T={c['T']:.3g} top_p={c['top_p']:.3g}: stats of "
                  f"{rows} rows checked, {n} requests restated, {amb} with more than one admissible outcome, "
                  f"0 tokens outside the admissible set")
    return n, amb


_custom_case, _random_case = sc.custom_case, sc.random_case


@pytest.mark.parametrize("name", list(sc.REAL_CASES))
def test_real_vocabulary_iteration_matches_the_oracle(name):
    """Row sampler, row stats and verify in the 1024-thread form (rows <= 512 and V >= 16384), the mixed launch (stats on
    256 threads, verify on 1024) and the 256-thread form on long rows (B > 512)."""
    c = sc.real_case(name)
    _check(c, _run_iteration(c), name)


def test_results_do_not_depend_on_the_thread_count():
    """K11: integer sums and order-free maxima.  The same rows at the same request indices in a batch of 8 (every
    kernel on 1024 threads) and embedded in a batch of 520 (every kernel on 256 threads): bit-identical."""
    big, small = sc.thread_count_cases()
    G, Bs = small["G"], small["B"]
    ob, os_ = _run_iteration(big), _run_iteration(small)
    _check(small, os_, "thread-count independence (1024 threads)")
    _check(big, ob, "thread-count independence (256 threads, long rows)")
    assert torch.equal(ob["rst_raw"][:Bs], os_["rst_raw"]) and torch.equal(ob["tst_raw"][:Bs * (G + 1)], os_["tst_raw"])
    assert np.array_equal(ob["drafts"][:Bs], os_["drafts"]) and np.array_equal(ob["tt"][:Bs], os_["tt"])
    assert np.array_equal(ob["ring"][:Bs], os_["ring"])


def test_draft_and_verify_graph_replays_equal_eager_iterations():
    V, B, G, K, T, top_p, seed = 128256, 4, 2, 4, 0.8, 0.9, 4242
    g = torch.Generator().manual_seed(12)
    tls = [(torch.randn(B * (G + 1), V, generator=g) * 2.5).to(torch.bfloat16) for _ in range(K)]
    dls = [[(tls[k].view(B, G + 1, V)[:, j].float() + torch.randn(B, V, generator=g) * 0.5).to(torch.bfloat16)
            for j in range(G)] for k in range(K)]

    def buffers():
        return dict(ctr=_counters(), ring=torch.zeros((B, G, V), dtype=torch.bfloat16, device=DEV),
                    rst=torch.zeros((B, G, 2), dtype=torch.int64, device=DEV),
                    tst=torch.zeros((B * (G + 1), 2), dtype=torch.int64, device=DEV),
                    tb=torch.full((B, G + 1), 3, dtype=torch.int64, device=DEV),
                    tok=torch.zeros((B, 1), dtype=torch.int64, device=DEV),
                    tt=torch.zeros((B, G + 1), dtype=torch.int64, device=DEV))

    def iteration(s, dx, tx):
        for j in range(G):
            ops.sample_rows(dx[j], 1, T, top_p, seed, ops.SAMPLE_DRAFT, s["ctr"], ops.ADVANCE_STEP, ring=s["ring"],
                            ring_stats=s["rst"], out=s["tok"])
            s["tb"][:, j + 1].copy_(s["tok"][:, 0])
        ops.spec_verify_sample(tx, s["tb"], s["ring"], s["rst"], s["tst"], s["ctr"], T, top_p, seed, out=s["tt"])

    s = buffers()
    dx = [torch.zeros((B, V), dtype=torch.bfloat16, device=DEV) for _ in range(G)]
    tx = torch.zeros((B * (G + 1), V), dtype=torch.bfloat16, device=DEV)
    for j in range(G):
        dx[j].copy_(dls[0][j])
    tx.copy_(tls[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        iteration(s, dx, tx)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    s["ctr"].zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        iteration(s, dx, tx)
    seen = set()
    for k in range(K):
        for j in range(G):
            dx[j].copy_(dls[k][j])
        tx.copy_(tls[k])
        graph.replay()
        torch.cuda.synchronize()
        e = buffers()
        e["ctr"][0] = k
        iteration(e, [x.to(DEV) for x in dls[k]], tls[k].to(DEV))
        torch.cuda.synchronize()
        for key in ("tt", "tb", "ring", "rst", "tst"):
            assert torch.equal(s[key], e[key]), (k, key)
        assert s["ctr"].tolist() == [k + 1, 0, 0, 0] == e["ctr"].tolist()
        seen.add(tuple(s["tt"].flatten().tolist()))
    assert s["ctr"].tolist() == [K, 0, 0, 0] and len(seen) == K


# ------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("name,V,pad", [("v32003_dense", 32003, None), ("v1001_dense", 1001, None),
                                        ("v32000_aligned_slice", 32000, (8, 24)),
                                        ("v32000_unaligned_slice", 32000, (3, 5)),
                                        ("v1001_unaligned_slice", 1001, (3, 5))])
def test_odd_vocabularies_unaligned_rows_and_strided_views(name, V, pad):
    """V not a multiple of 8: rows after the first are not 16-byte aligned and the scalar tail of for_row / draw_row
    is live.  row_stride > vocab: a column slice of a wider tensor (aligned start and aligned stride, or neither), for
    the draft launches and the verify alike; the ring stays contiguous."""
    c = _random_case(name, V, 6, 2, 0.7, 0.9, 0.6, pad=pad)
    _check(c, _run_iteration(c), name)


def _draw_rows(rows_f32, T, top_p, seed=321, it=6, N=None):
    """One draft-mode launch over rows [B, V] (or one row for N requests, stride 0) -> (tokens, Rows checked)."""
    xb = rows_f32.to(torch.bfloat16)
    B, V = xb.shape if N is None else (N, xb.shape[-1])
    x = xb.to(DEV) if N is None else xb.to(DEV).view(1, V).expand(N, V)
    ctr = _counters()
    ctr[0] = it
    ring = torch.zeros((B, 1, V), dtype=torch.bfloat16, device=DEV)
    rst = torch.zeros((B, 1, 2), dtype=torch.int64, device=DEV)
    tok = ops.sample_rows(x, 1, T, top_p, seed, ops.SAMPLE_DRAFT, ctr, ops.ADVANCE_STEP, ring=ring, ring_stats=rst)
    torch.cuda.synchronize()
    tok = tok[:, 0].cpu().numpy()
    st = _stats_np(rst)
    bits = sc.bits_of(xb.view(-1, V))
    rows = []
    for b in range(B if N is None else min(N, 16)):
        row = sr.check_stats(bits[b if N is None else 0], T, top_p, *(a[b] for a in st), tag=f"row {b}")
        adm = sr.draw_admissible(row, seed, sr.DRAFT, 0, b, it)
        assert tok[b] in adm, (b, tok[b], adm)
        rows.append(row)
    return tok, rows, st


@pytest.mark.parametrize("V", [1001, 32000])
def test_row_sampler_with_minus_infinity_entries(V):
    g = torch.Generator().manual_seed(V)
    x = torch.randn(6, V, generator=g) * 2
    x[0, 100:900] = float("-inf")                       # a span
    x[1, ::2] = float("-inf")                           # a masked vocabulary
    x[2, : V - 3] = float("-inf")                       # only the scalar tail / last lanes are alive
    x[3] = float("-inf")
    x[3, V // 2 + 1] = -2.5                              # all but one
    x[4, :] = float("-inf")
    x[4, 0] = 7.0
    for top_p in (0.9, 1.0):
        tok, rows, (m, kstar, zk) = _draw_rows(x, 0.8, top_p)
        assert not torch.isinf(x[torch.arange(6), torch.from_numpy(tok)]).any()
        assert tok[3] == V // 2 + 1 and tok[4] == 0     # forced
        for b, val in ((3, -2.5), (4, 7.0)):
            assert m[b] == np.float32(val) and zk[b] == 2 ** 40          # p~ = 1
            if top_p < 1:
                assert kstar[b] == int(sr.key16(sr.bf16_bits(np.float32(val))))
    parity_report(f"[sampling] -inf entries V={V}: 6 rows x 2 top_p, stats exact, tokens admissible, forced tokens forced")


def test_all_equal_row_keeps_every_token_for_any_top_p():
    V, N = 50, 1 << 16
    for top_p in (0.3, 1e-6):
        tok, rows, (m, kstar, zk) = _draw_rows(torch.full((1, V), 1.25), 0.9, top_p, N=N)
        assert (kstar == int(sr.key16(sr.bf16_bits(np.float32(1.25))))).all() and (zk == V * 2 ** 40).all()
        ok, pval = _chi2_ok(np.bincount(tok, minlength=V), np.full(V, 1.0 / V))
        assert ok, (top_p, pval)


def test_tie_group_across_the_top_p_boundary_is_kept_whole_on_the_gpu():
    vals = torch.tensor([3.0] * 1 + [2.0] * 6 + [0.0] * 20).view(1, -1)     # test_top_p_keeps_or_drops_a_tie_group_whole
    N = 1 << 14
    tok, rows, (m, kstar, zk) = _draw_rows(vals, 1.0, 0.5, N=N)
    assert (kstar == int(sr.key16(sr.bf16_bits(np.float32(2.0))))).all()
    counts = np.bincount(tok, minlength=27)
    assert counts[7:].sum() == 0 and (counts[:7] > 0).all()
    ok, pval = _chi2_ok(counts, rows[0].p)
    assert ok, pval
    tok, _, (m, kstar, zk) = _draw_rows(vals, 1.0, 0.01, N=N)
    assert (tok == 0).all() and (zk == 2 ** 40).all()


def test_signed_zeros_have_distinct_keys_at_the_boundary():
    vals = torch.tensor([0.0, -0.0] + [-5.0] * 20).view(1, -1)             # masses 1, 1, 20 e^-5 = 0.135
    N = 1 << 12
    tok, _, (m, kstar, zk) = _draw_rows(vals, 1.0, 0.3, N=N)                # mass above -0 is 1 > 0.3 Z: -0 is dropped
    assert (kstar == 0x8000).all() and (tok == 0).all() and (zk == 2 ** 40).all()
    tok, _, (m, kstar, zk) = _draw_rows(vals, 1.0, 0.6, N=N)                # 1 <= 0.6 Z = 1.28 < 2: -0 kept, -5 dropped
    assert (kstar == 0x7FFF).all() and (zk == 2 ** 41).all()
    counts = np.bincount(tok, minlength=22)
    assert counts[2:].sum() == 0 and counts[0] > N // 3 and counts[1] > N // 3
    # the compare is "<=" (K11), on a case where it is exact: masses 2^40 and 2^40 (both exp(0)), the rest 0, top_p = 1/2
    # (1/4 with three -0): the mass above -0 EQUALS top_p Z = 2^40 in the kernel's double compare, so -0 is kept
    for n_neg, top_p in ((1, 0.5), (3, 0.25)):
        vals = torch.tensor([0.0] + [-0.0] * n_neg + [float("-inf")] * 20).view(1, -1)
        tok, _, (m, kstar, zk) = _draw_rows(vals, 0.7, top_p, N=N)
        assert (kstar == 0x7FFF).all() and (zk == (1 + n_neg) * 2 ** 40).all()
        counts = np.bincount(tok, minlength=22)
        assert counts[1 + n_neg:].sum() == 0 and (counts[:1 + n_neg] > 0).all()


def test_tiny_top_p_keeps_only_the_maximal_tie_group():
    V = 32000
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, V, generator=g) * 2
    top = float(x.max()) + 1.0
    groups = [[5], [V - 1, 17, 4000], [8, 9], [31999, 31998, 31997, 0]]
    for b, idx in enumerate(groups):
        x[b, idx] = top
    for rep in range(3):
        tok, rows, (m, kstar, zk) = _draw_rows(x, 0.7, 1e-6, it=rep)
        for b, idx in enumerate(groups):
            assert tok[b] in idx and zk[b] == len(idx) * 2 ** 40 and rows[b].keep.sum() == len(idx)


@pytest.mark.parametrize("name,V,T,scale", [("T0.05_most_masses_zero", 32000, 0.05, 2.5),
                                            ("T50_all_masses_near_2^40", 151936, 50.0, 1.0)])
def test_temperature_extremes(name, V, T, scale):
    c = _random_case(name, V, 4, 2, T, 0.9, 0.4, scale=scale)
    o = _run_iteration(c)
    _check(c, o, name)
    zk = np.concatenate([o["rst"][2], o["tst"][2]]).astype(np.float64)
    if T > 1:
        assert zk.min() > 0.5 * V * 2.0 ** 40 and zk.max() < 2.0 ** 58        # mass_fx's comment: the row sums below 2^58
    else:
        assert zk.max() < 64 * 2.0 ** 40


def _first_rejection(tt, tokens, V):
    G = tt.shape[1] - 1
    jr = np.full(len(tt), G)
    for b in range(len(tt)):
        for j in range(G):
            if tt[b, j] != tokens[b, j + 1] or not 0 <= tokens[b, j + 1] < V:
                jr[b] = j
                break
    return jr


@pytest.mark.parametrize("V", [1001, 32000])
def test_out_of_range_draft_tokens_are_rejections(V):
    """d = -1 and d = vocab at position 0 and at a later one: jr is that position (unless an earlier draft was rejected
    anyway -- then nothing changes), earlier accepted drafts are kept, the corrected token is an admissible residual
    draw that excludes nothing real."""
    B, G = 16, 3
    c = _random_case(f"out_of_range_{V}", V, B, G, 0.8, 0.9, 0.3)
    clean = _run_iteration(c)
    _check(c, clean, f"out-of-range drafts V={V} (clean run)")
    jr_clean = _first_rejection(clean["tt"], clean["tokens"], V)
    plan = [(b, (0, 2, 1, 2)[b % 4], (-1, V)[(b // 4) % 2]) for b in range(B)]

    def edit(tb):
        for b, pos, bad in plan:
            tb[b, pos + 1] = bad
    o = _run_iteration(c, tokens_edit=edit)
    _check(c, o, f"out-of-range drafts V={V}")
    assert np.array_equal(o["drafts"], clean["drafts"])
    hit = 0
    for b, pos, bad in plan:
        if jr_clean[b] < pos:
            assert np.array_equal(o["tt"][b], clean["tt"][b])
            continue
        hit += 1
        assert np.array_equal(o["tt"][b, :pos], clean["drafts"][b, :pos])
        assert 0 <= o["tt"][b, pos] < V and (o["tt"][b, pos + 1:] == -1).all()
    assert hit >= B // 4


@pytest.mark.parametrize("V", [1001, 32000])
def test_zero_residual_fallback_and_matching_rows_accept_every_valid_draft(V):
    """The "draft" is drawn from the target logits, so ring rows and stats are bit-identical to the target's.  Valid
    drafts: every one is accepted (u < 1) and the bonus is an admissible draw.  An out-of-range d at a position: the
    residual is zero everywhere and the token is a draw from p~ under the RESIDUAL key (the oracle knows r == 0 exactly
    where both sides are the same function of the same bits)."""
    B, G = 12, 3
    c = _random_case(f"fallback_{V}", V, B, G, 0.9, 0.9, 0.0)
    o = _run_iteration(c)
    _check(c, o, f"ring == target, valid drafts V={V}")
    assert torch.equal(o["rst_raw"].view(B, G, 2), o["tst_raw"].view(B, G + 1, 2)[:, :G])
    assert np.array_equal(o["tt"][:, :G], o["drafts"]) and (o["tt"][:, G] >= 0).all()
    plan = [(b, b % G, (-1, V)[b % 2]) for b in range(B)]

    def edit(tb):
        for b, pos, bad in plan:
            tb[b, pos + 1] = bad
    f = _run_iteration(c, tokens_edit=edit)
    n, amb = _check(c, f, f"zero-residual fallback V={V}")
    tb_bits = sc.bits_of(c["tl"])
    for b, pos, bad in plan:
        assert np.array_equal(f["tt"][b, :pos], o["drafts"][b, :pos]) and (f["tt"][b, pos + 1:] == -1).all()
        row = sr.check_stats(tb_bits[b, pos], c["T"], c["top_p"], *(a[b * (G + 1) + pos] for a in f["tst"]))
        assert f["tt"][b, pos] in sr.draw_admissible(row, c["seed"], sr.RESIDUAL, pos, b, c["it"], exclude=bad)


def test_zero_residual_fallback_follows_the_filtered_target_distribution():
    V, N, T, top_p = 50, 1 << 16, 1.0, 0.9
    g = torch.Generator().manual_seed(21)
    row = torch.randn(1, 1, V, generator=g) * 1.5
    c = _custom_case("fallback_chi2", row.expand(N, 2, V), row.expand(N, 1, V), T, top_p, restate=list(range(48)))

    def edit(tb):
        tb[:, 1] = -1
    o = _run_iteration(c, tokens_edit=edit)
    n = 48                                              # the oracle on the first requests, the distribution over all
    head = dict(c, B=n, tl=c["tl"][:n], dl=[x[:n] for x in c["dl"]], tok0=c["tok0"][:n])
    _check(head, dict(o, ring=o["ring"][:n], rst=[a[:n] for a in o["rst"]], tst=[a[:2 * n] for a in o["tst"]],
                      drafts=o["drafts"][:n], tt=o["tt"][:n], tokens=o["tokens"][:n]),
           f"zero-residual fallback, chi-square over {N} requests")
    assert (o["tt"][:, 1] == -1).all()
    ok, pval = _chi2_ok(np.bincount(o["tt"][:, 0], minlength=V), _filtered(row[0, 0], T, top_p))
    assert ok, pval


def test_fallback_with_a_rejected_in_range_draft_never_returns_it():
    """The fallback with a real d needs u q~(d) >= p~(d) while p~ <= q~ everywhere: handed a ring whose stored zkept is
    half the target's (q~ = 2 p~ on the same bits; the verify reads the stats it is given), half of the requests reject
    with a residual that is zero everywhere.  The corrected token is then a draw from p~ WITHOUT d."""
    V, N, T, top_p = 50, 1 << 12, 1.0, 0.9
    g = torch.Generator().manual_seed(22)
    row = torch.randn(1, 1, V, generator=g) * 1.5
    c = _custom_case("fallback_in_range", row.expand(N, 2, V), row.expand(N, 1, V), T, top_p, restate=[])

    def halve(rst):
        rst[:, :, 1] //= 2
    o = _run_iteration(c, ring_stats_edit=halve)
    tt, d = o["tt"], o["drafts"][:, 0]
    rejected = tt[:, 1] == -1
    assert 0.4 * N < rejected.sum() < 0.6 * N
    assert (tt[~rejected, 0] == d[~rejected]).all()
    assert (tt[rejected, 0] != d[rejected]).all(), "the fallback drew the rejected draft token"
    bits = sc.bits_of(c["tl"])
    P = sr.check_stats(bits[0, 0], T, top_p, *(a[0] for a in o["tst"]))
    Q = sr.Row(bits[0, 0], T, P.m, P.kstar, P.zkept // 2)
    checked = 0
    for b in range(128):
        outs = sr.verify_admissible([P, P], [Q], o["tokens"][b], c["seed"], b, c["it"])
        assert sr.contains(outs, tt[b]), (b, tt[b], outs)
        if rejected[b]:
            assert tt[b, 0] in sr.draw_admissible(P, c["seed"], sr.RESIDUAL, 0, b, c["it"], exclude=int(d[b]))
            checked += 1
    assert checked > 32
    parity_report(f"[sampling] fallback with an in-range rejected draft: {int(rejected.sum())} of {N} requests rejected, "
                  f"none returned d; 128 requests restated, 0 outside the admissible set")


def _accept_kernel_equals_cpu(tokens, tt, G, eot_1, eot_2):
    """ops.accept_rollback and tests/cpu_ops.accept_rollback on the same tokens_buffer / target_tokens (host arrays):
    every piece of state equal -> the device state."""
    from tests import cpu_ops
    B = len(tokens)
    tb, tt = torch.from_numpy(tokens).clone(), torch.from_numpy(tt).clone()

    def state():
        return dict(out=torch.zeros((B, 64), dtype=torch.long), num_nodes=torch.full((B,), 20, dtype=torch.long),
                    cachelens=torch.full((B,), 20 + G + 1, dtype=torch.int32),
                    lpl=torch.full((B,), 20 + G + 1, dtype=torch.int32), an=torch.zeros(B, dtype=torch.long),
                    bonus=torch.zeros(B, dtype=torch.long), dbl=torch.zeros((B, 2), dtype=torch.long),
                    cu=torch.ones(B, dtype=torch.long), flags=torch.zeros(2, dtype=torch.int32))
    h, d = state(), {k: v.to(DEV) for k, v in state().items()}
    tbc, tbd = tb.clone(), tb.to(DEV)
    cpu_ops.accept_rollback(tbc, tt, h["out"], h["num_nodes"], h["cachelens"], h["lpl"], None, None, G, G, G,
                            eot_1, eot_2, 10 ** 6, h["an"], h["bonus"], h["dbl"], h["cu"], h["flags"])
    ops.accept_rollback(tbd, tt.to(DEV), d["out"], d["num_nodes"], d["cachelens"], d["lpl"], None, None, G, G, G, eot_1,
                        eot_2, 10 ** 6, d["an"], d["bonus"], d["dbl"], d["cu"], d["flags"])
    torch.cuda.synchronize()
    for k in h:
        assert torch.equal(h[k], d[k].cpu()), k
    assert torch.equal(tbc, tbd.cpu())
    return d


def test_verify_then_accept_kernel_cuts_at_an_end_of_text_draft():
    c, eot_1, eot_2, expect = sc.eot_case()
    assert expect, "no request has an end-of-text token among its accepted drafts"
    B, G = c["B"], c["G"]
    o = _run_iteration(c)
    _check(c, o, "end-of-text among accepted drafts")
    d = _accept_kernel_equals_cpu(o["tokens"], o["tt"], G, eot_1, eot_2)
    # ring == target: every draft is accepted by the verify, so the cut is at the first end-of-text draft exactly
    assert np.array_equal(o["tt"][:, :G], o["drafts"])
    for b, pos in expect.items():
        assert np.array_equal(o["drafts"][b], c["cpu_drafts"][b])
    an = d["an"].cpu()
    for b in range(B):
        eot = [j for j in range(G) if o["drafts"][b, j] in (eot_1, eot_2)]
        assert int(an[b]) == (eot[0] + 1 if eot else G + 1), (b, o["drafts"][b], int(an[b]))
        if eot:
            assert int(d["bonus"][b]) == o["drafts"][b, eot[0]]
    assert int(d["flags"][0]) == 1


def test_non_contiguous_tokens_buffer_is_copied_and_read_correctly():
    c = _random_case("noncontiguous_tb", 2048, 8, 3, 0.8, 0.9, 0.5)
    o = _run_iteration(c)
    B, G, V = c["B"], c["G"], c["V"]
    wide_tb = torch.full((B, 2 * (G + 1)), -7, dtype=torch.int64, device=DEV)
    view = wide_tb[:, ::2]
    view.copy_(torch.from_numpy(o["tokens"]).to(DEV))
    assert not view.is_contiguous()
    ctr = _counters()
    ctr[0] = c["it"]
    ring = torch.from_numpy(o["ring"].view(np.int16)).view(torch.bfloat16).to(DEV)
    tst = torch.zeros((B * (G + 1), 2), dtype=torch.int64, device=DEV)
    tt = ops.spec_verify_sample(c["tl"].reshape(B * (G + 1), V).to(DEV), view, ring, o["rst_raw"].to(DEV), tst, ctr,
                                c["T"], c["top_p"], c["seed"])
    torch.cuda.synchronize()
    assert np.array_equal(tt.cpu().numpy(), o["tt"]) and torch.equal(tst.cpu(), o["tst_raw"])


def test_sampling_rejects_bad_arguments():
    B, G, V = 4, 2, 64
    x = torch.zeros((B, V), dtype=torch.bfloat16, device=DEV)
    xv = torch.zeros((B * (G + 1), V), dtype=torch.bfloat16, device=DEV)
    ctr = _counters()
    ring = torch.zeros((B, G, V), dtype=torch.bfloat16, device=DEV)
    rst = torch.zeros((B, G, 2), dtype=torch.int64, device=DEV)
    tst = torch.zeros((B * (G + 1), 2), dtype=torch.int64, device=DEV)
    tb = torch.zeros((B, G + 1), dtype=torch.int64, device=DEV)
    err = (ValueError, ops.MagicDecHipError)

    def draw(logits=x, T=1.0, top_p=0.9, ctr=ctr, **kw):
        return ops.sample_rows(logits, 1, T, top_p, 1, ops.SAMPLE_DRAFT, ctr, ops.ADVANCE_STEP, **kw)

    def verify(logits=xv, tb=tb, ring=ring, rst=rst, tst=tst, ctr=ctr, T=1.0, top_p=0.9):
        return ops.spec_verify_sample(logits, tb, ring, rst, tst, ctr, T, top_p, 1)

    bad = [lambda: draw(T=0.0), lambda: draw(T=-1.0), lambda: draw(top_p=0.0), lambda: draw(top_p=1.5),
           lambda: verify(T=0.0), lambda: verify(top_p=0.0), lambda: verify(top_p=1.0001),
           lambda: draw(ring=ring), lambda: draw(ring_stats=rst),                       # ring without stats and back
           lambda: draw(ring=ring[:, :0], ring_stats=rst[:, :0]),                       # gamma = 0 with a ring
           lambda: verify(logits=xv[:1].expand(B * (G + 1), V)),                        # row_stride (0) < vocab
           lambda: draw(ring=ring[:, :, : V - 8].contiguous(), ring_stats=rst),         # ring vocabulary
           lambda: draw(ring=ring[: B - 1], ring_stats=rst[: B - 1]),                   # ring batch
           lambda: draw(ring=ring, ring_stats=rst[:, :1]),                              # stats shape
           lambda: verify(logits=xv[: B * G]), lambda: verify(ring=ring[:, :1]), lambda: verify(tb=tb[:, :G]),
           lambda: verify(rst=rst[:, :1]), lambda: verify(tst=tst[:B]),
           lambda: draw(logits=x.float()), lambda: verify(logits=xv.float()),           # dtypes
           lambda: draw(ring=ring.float(), ring_stats=rst), lambda: verify(ring=ring.to(torch.float16)),
           lambda: verify(tb=tb.int()), lambda: verify(rst=rst.int()), lambda: verify(tst=tst.int()),
           lambda: draw(ctr=ctr.long()), lambda: verify(ctr=ctr.long()),
           lambda: draw(ring=ring, ring_stats=rst.int()),
           lambda: draw(row_sel=torch.ones(B, dtype=torch.int32, device=DEV)),
           lambda: draw(logits=x[:, ::2]),                                               # inner stride
           lambda: draw(logits=x.cpu())]
    for i, f in enumerate(bad):
        with pytest.raises(err):
            f()
            pytest.fail(f"bad call {i} was accepted")
    torch.cuda.synchronize()
    assert ctr.tolist() == [0, 0, 0, 0]                  # nothing was launched: no launch advanced or ticketed
    draw(ring=ring, ring_stats=rst)                      # and the good calls still go through
    verify()
    torch.cuda.synchronize()
