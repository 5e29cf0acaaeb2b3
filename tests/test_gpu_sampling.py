"""GPU tests of the sampling kernels (csrc/sample.hip, include/magicdec_hip.h K11) through the C ABI: the row sampler
against the numpy restatement (tests/sampling_ref.py), determinism and graph replays, the drawn distribution, the
lossless speculative verify, and the verify kernel followed by the unchanged accept kernel."""
import numpy as np
import pytest
import torch

from magicdec_amd import ops
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
