"""Inputs of the sampling tests that run on the GPU (tests/test_gpu_sampling.py, tests/test_gpu_fuzz.py) and the
oracle-side checks of one draft / verify iteration -- shared with tests/test_sampling_cpu.py, which runs the
admissible-outcome oracle of tests/sampling_ref.py over the very same fixed-seed inputs without a GPU to show that they
leave (almost) no request ambiguous.  Everything here is torch-on-CPU / numpy."""
from __future__ import annotations

import math
import random

import numpy as np
import torch

from tests import sampling_ref as sr

BF = torch.bfloat16
SEED = 0x5EED_0123_4567

# name -> (V, B, gamma, T, top_p, sigma, scale, iteration): the real-vocabulary cases.  wide(rows, V) of csrc/sample.hip
# picks 1024 threads iff rows <= 512 and V >= 16384, the stats kernel with rows = B (gamma + 1), the row sampler and the
# verify kernel with rows = B.
REAL_CASES = {
    "v32000_all1024": (32000, 32, 3, 0.6, 0.9, 0.5, 2.5, 3),
    "v128256_all1024_top_p1": (128256, 32, 3, 0.6, 1.0, 0.5, 2.5, 3),
    "v151936_all1024_gamma5": (151936, 16, 5, 1.0, 0.95, 0.3, 2.5, 11),
    "v128256_all1024_gamma1": (128256, 20, 1, 1.5, 0.8, 1.0, 2.0, 70000),
    "v32000_mixed_stats256_verify1024": (32000, 160, 3, 0.8, 0.9, 0.7, 2.5, 5),
    "v16384_all256_long_rows": (16384, 520, 1, 0.7, 0.95, 0.5, 2.5, 9),
}
MAX_RESTATED = 32


def bits_of(t):
    """bf16 tensor -> uint16 numpy array of its bit patterns."""
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def subset(B, limit, seed):
    """The seeded subset of requests whose tokens are restated (all of them when B <= limit)."""
    if B <= limit:
        return list(range(B))
    return sorted(random.Random(seed).sample(range(B), limit))


def real_case(name):
    V, B, G, T, top_p, sigma, scale, it = REAL_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    tl = (torch.randn(B, G + 1, V, generator=g) * scale).to(BF)
    dl = (tl[:, :G].float() + torch.randn(B, G, V, generator=g) * sigma).to(BF)
    return dict(name=name, V=V, B=B, G=G, T=T, top_p=top_p, it=it, seed=SEED, tl=tl,
                dl=[dl[:, j:j + 1].contiguous() for j in range(G)], row_sel=None,
                tok0=torch.randint(0, V, (B,), generator=g), pad=None, eot=(-5, -6),
                restate=subset(B, MAX_RESTATED, B))


FUZZ_DEFAULT = 10
FUZZ_V = [50, 1001, 2048, 16384, 32003, 128256]


def fuzz_case(seed):
    """Every draw of fuzz case `seed` (tests/test_gpu_fuzz.py::test_fuzz_sampling_vs_restatement)."""
    r = random.Random(13000 + seed)
    V = r.choice(FUZZ_V)
    B = r.randint(1, 12 if V > 100000 else (32 if V >= 16384 else 48))
    if r.random() < 0.1:
        B, V = r.randint(513, 560), r.choice([50, 1001, 2048])
    G = r.randint(1, 5)
    T = math.exp(r.uniform(math.log(0.2), math.log(3.0)))
    top_p = 1.0 if r.random() < 0.3 else r.uniform(0.3, 0.99)
    scale = r.choice([0.5, 1.5, 2.5, 4.0])
    sigma = r.choice([0.0, 0.0, 0.2, 0.5, 1.0, 2.0])
    n0 = r.choice([1, 2])
    g = torch.Generator().manual_seed(13000 + seed)
    tl = torch.randn(B, G + 1, V, generator=g) * scale
    dl = [tl[:, j:j + 1] + torch.randn(B, 1, V, generator=g) * sigma for j in range(G)]
    row_sel = None
    if n0 == 2:
        row_sel = torch.randint(1, 3, (B,), generator=g)
        other = torch.randn(B, 1, V, generator=g) * scale            # the row of the two-token step that is NOT drawn
        first = torch.where((row_sel == 1).view(B, 1, 1), dl[0], other)
        second = torch.where((row_sel == 2).view(B, 1, 1), dl[0], other)
        dl[0] = torch.cat([first, second], dim=1)
    # planted structure, the same in the target row and the draft row it is verified against
    for _ in range(r.randint(0, 3)):
        b, j = r.randrange(B), r.randrange(G)
        kind = r.choice(["ties", "neginf", "peak"])
        rows = [tl[b, j]] + [dl[j][b, i] for i in range(dl[j].shape[1])]
        if kind == "ties":
            idx = torch.randperm(V, generator=g)[: r.randint(2, max(2, V // 3))]
            val = float(tl[b, j].max()) - r.choice([0.0, 0.5, 2.0])
            for row in rows:
                row[idx] = val
        elif kind == "neginf":
            a = r.randrange(V)
            e = min(V, a + r.randint(1, max(1, V // 2)))
            for row in rows:
                row[a:e] = float("-inf")
            if not torch.isfinite(tl[b, j]).any():
                tl[b, j, 0] = 0.0
        else:
            v = r.randrange(V)
            for row in rows:
                row[v] = float(row[torch.isfinite(row)].max()) + 3.0
    for row in [tl[b, j] for b in range(B) for j in range(G + 1)] + [x[b, i] for x in dl for b in range(B)
                                                                     for i in range(x.shape[1])]:
        if not torch.isfinite(row).any():                              # a wholly -inf row is outside K11
            row[0] = 0.0
    pad = None if r.random() < 0.5 else (r.choice([0, 3, 8]), r.choice([5, 8, 64]))
    return dict(name=f"fuzz{seed}", V=V, B=B, G=G, T=T, top_p=top_p, it=r.randint(0, 2 ** 30), seed=r.getrandbits(64),
                tl=tl.to(BF), dl=[x.to(BF).contiguous() for x in dl], row_sel=row_sel,
                tok0=torch.randint(0, V, (B,), generator=g), pad=pad, eot=(r.randrange(V), r.randrange(V)),
                restate=subset(B, 4 if V >= 16384 else 10, seed))


def drawn_rows(c):
    """[B, gamma, V] bf16: the draft row each step draws from (row row_sel - 1 of the two-token step, else the last)."""
    rows = []
    for x in c["dl"]:
        if x.shape[1] == 1:
            rows.append(x[:, 0])
        else:
            sel = c["row_sel"] if c["row_sel"] is not None else torch.full((c["B"],), x.shape[1])
            rows.append(x[torch.arange(c["B"]), sel - 1])
    return torch.stack(rows, dim=1)


def cpu_iteration(c):
    """The iteration of case `c` by the restatement alone (its own statistics, its own float64 draft draws) ->
    (requests restated, requests with more than one admissible outcome, requests whose float64 outcome is missing from
    the admissible set)."""
    T, top_p, seed, it, G = c["T"], c["top_p"], c["seed"], c["it"], c["G"]
    tb, rb = bits_of(c["tl"]), bits_of(drawn_rows(c))
    ambiguous = missing = 0
    for b in c["restate"]:
        rrows = [sr.ref_row(rb[b, j], T, top_p) for j in range(G)]
        trows = [sr.ref_row(tb[b, j], T, top_p) for j in range(G + 1)]
        tokens, multi = [int(c["tok0"][b])], False
        for j in range(G):
            adm = sr.draw_admissible(rrows[j], seed, sr.DRAFT, j, b, it)
            multi |= len(adm) > 1
            tokens.append(int(sr.draw_admissible(rrows[j], seed, sr.DRAFT, j, b, it, widen=0.0)[0]))
        outs = sr.verify_admissible(trows, rrows, tokens, seed, b, it)
        exact = sr.verify_admissible(trows, rrows, tokens, seed, b, it, widen=0.0)
        missing += not (len(exact) == 1 and sr.contains(outs, exact[0]))
        ambiguous += bool(multi or len(outs) > 1)
    return len(c["restate"]), ambiguous, missing


def check_iteration(c, ring, ring_stats, target_stats, drafts, tt, tokens=None):
    """Kernel outputs of one iteration of case `c` against the oracle.  ring [B, gamma, V] uint16 bits, ring_stats /
    target_stats = (m, kstar, zkept) arrays over [B * gamma] / [B * (gamma + 1)] rows, drafts [B, gamma] the tokens the
    draft launches returned, tt [B, gamma + 1] the verify's target_tokens, tokens [B, gamma + 1] the tokens_buffer the
    verify read (default: tok0 | drafts).  Asserts: ring rows bit for bit; the stats of ALL rows; the -1 fill of all
    requests; draft tokens and target_tokens of the restated requests by membership.  -> (restated, ambiguous)."""
    T, top_p, seed, it, G, B = c["T"], c["top_p"], c["seed"], c["it"], c["G"], c["B"]
    tag = c["name"]
    tb, rb = bits_of(c["tl"]), bits_of(drawn_rows(c))
    assert np.array_equal(ring, rb), f"{tag}: the ring is not the drawn draft rows"
    if tokens is None:
        tokens = np.concatenate([c["tok0"].numpy().reshape(B, 1), drafts], axis=1)
    restate = set(c["restate"])
    ambiguous = 0
    for b in range(B):
        rrows = [sr.check_stats(rb[b, j], T, top_p, *(a[b * G + j] for a in ring_stats), tag=f"{tag} ring[{b},{j}]")
                 for j in range(G)]
        trows = [sr.check_stats(tb[b, j], T, top_p, *(a[b * (G + 1) + j] for a in target_stats),
                                tag=f"{tag} target[{b},{j}]") for j in range(G + 1)]
        jr = G
        for j in range(G):
            if tt[b, j] != tokens[b, j + 1] or not 0 <= tokens[b, j + 1] < c["V"]:
                jr = j
                break
        assert 0 <= tt[b, jr] < c["V"] and (tt[b, jr + 1:] == -1).all(), f"{tag}: request {b}: {tt[b].tolist()}"
        if b not in restate:
            continue
        multi = False
        for j in range(G):
            adm = sr.draw_admissible(rrows[j], seed, sr.DRAFT, j, b, it)
            assert drafts[b, j] in adm, f"{tag}: draft token [{b},{j}] = {drafts[b, j]}, admissible {adm.tolist()}"
            multi |= len(adm) > 1
        outs = sr.verify_admissible(trows, rrows, tokens[b], seed, b, it)
        assert sr.contains(outs, tt[b]), (f"{tag}: request {b}: target_tokens {tt[b].tolist()} not admissible "
                                          f"{[o.tolist() for o in outs[:8]]} (tokens_buffer {tokens[b].tolist()})")
        ambiguous += bool(multi or len(outs) > 1)
    return len(restate), ambiguous


def eot_case():
    """ring == target at V = 1000 (every draft is accepted), with the end-of-text ids chosen among the restatement's own
    draft tokens -> (case, eot_1, eot_2, {request: position of its first end-of-text draft}); the requests listed have
    exactly one admissible token at every draft step."""
    V, B, G, T, top_p = 1000, 48, 3, 0.8, 0.9
    g = torch.Generator().manual_seed(77)
    tl = (torch.randn(B, G + 1, V, generator=g) * 2.5).to(BF)
    c = dict(name="eot", V=V, B=B, G=G, T=T, top_p=top_p, it=21, seed=SEED, tl=tl,
             dl=[tl[:, j:j + 1].contiguous() for j in range(G)], row_sel=None,
             tok0=torch.randint(0, V, (B,), generator=g), pad=None, restate=list(range(B)))
    rb = bits_of(drawn_rows(c))
    drafts = np.zeros((B, G), dtype=np.int64)
    single = np.ones(B, dtype=bool)
    for b in range(B):
        for j in range(G):
            adm = sr.draw_admissible(sr.ref_row(rb[b, j], T, top_p), c["seed"], sr.DRAFT, j, b, c["it"])
            drafts[b, j] = adm[0]
            single[b] &= len(adm) == 1
    eot_1, eot_2 = int(drafts[2, 1]), int(drafts[7, 0])
    expect = {}
    for b in range(B):
        pos = [j for j in range(G) if drafts[b, j] in (eot_1, eot_2)]
        if pos and single[b]:
            expect[b] = pos[0]
    c["cpu_drafts"], c["eot"] = drafts, (eot_1, eot_2)
    return c, eot_1, eot_2, expect


def custom_case(name, tl, dl, T, top_p, it=4, pad=None, seed=SEED, restate=None):
    """tl [B, G+1, V], dl [B, G, V] float32 -> a case dict in the form of real_case()."""
    B, G1, V = tl.shape
    return dict(name=name, V=V, B=B, G=G1 - 1, T=T, top_p=top_p, it=it, seed=seed, tl=tl.to(BF),
                dl=[dl[:, j:j + 1].to(BF).contiguous() for j in range(G1 - 1)], row_sel=None,
                tok0=torch.arange(B) % V, pad=pad, eot=(-5, -6),
                restate=list(range(B)) if restate is None else restate)


def random_case(name, V, B, G, T, top_p, sigma, scale=2.5, **kw):
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    tl = torch.randn(B, G + 1, V, generator=g) * scale
    dl = tl[:, :G] + torch.randn(B, G, V, generator=g) * sigma
    return custom_case(name, tl, dl, T, top_p, **kw)


def thread_count_cases():
    """The same rows at the same request indices in a batch of 8 (every kernel on 1024 threads) and embedded in a batch
    of 520 (every kernel on 256 threads) -> (big, small); the 8 shared requests are the restated ones of both."""
    V, G, Bs, Bb = 16384, 2, 8, 520
    big = random_case("thread_count", V, Bb, G, 0.7, 0.9, 0.6, restate=list(range(Bs)))
    small = dict(big, B=Bs, tl=big["tl"][:Bs], dl=[x[:Bs] for x in big["dl"]], tok0=big["tok0"][:Bs])
    return big, small
