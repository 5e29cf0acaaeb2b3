"""Score regimes for the attention kernels (CPU only, deterministic): inputs whose softmax scores are NOT N(0, 1).

Every other attention test draws q, K, V = randn with sm_scale = 1/sqrt(D): max |s| ~ 4.5 nats, largest probability of a
row ~ 0.016, every running maximum within a few units of every other -- so ANY reference maximum (slot 0's, a stale
one, a wrong initial value) gives the right answer, and one leaked key moves the output by |v|/L, far below the gate.
The regimes below separate a correct (m, l, O) merge from one that overflows, underflows or takes the wrong maximum,
and make a single leaked key or an ignored sm_scale change whole output rows:

  randn            today's baseline (contrast line of the report)
  ints2/4/8        integer q, K in [-amp, amp]: every q.k is an exact integer in any summation order
  wide             randn q * 8, K * 4: non-integer, std ~ 30 nats at the default scale
  mixed            ints2 keys, every 7th key row x 16, every 5th x 2^-12
  sink             key 0 carries about half the mass of every row
  late-peak        the same key placed last (the last key every row of the chunk sees): the accumulator is rescaled by
                   ~0 on the final tile
  rising           score shift grows linearly with the position (>= 300 nats from 200 keys on): the running maximum moves on every tile
  falling          the mirror image: maximum set in tile 0, late tiles underflow
  offset           every score near -400 nats: the result must not depend on where zero is
  saturated        (saturated_request) every query row has ONE key that beats every other visible key by >= 160 in log2
                   units: every other exp2 is exactly 0 in fp32 and the row's output must equal that key's V row bit for
                   bit.  Keys one past a row's causal limit hold a twice-stronger key of that row (a trap): a mask that
                   leaks one key flips the row to another V row at any context length.

The structured regimes (sink .. offset) add multiples of one fixed +-1 direction u to randn q / K whose u component
was projected out: the score shift of key i is a * c_i * |u|^2 * sm_scale up to the bf16 rounding of the inputs, and q
is pre-scaled by 1 / (sqrt(D) sm_scale), so these regimes present the same scores at every sm_scale (a kernel that ignores
the parameter fails them).  The wide regimes are not compensated: their declared bands scale with sm_scale.

What a test may assert is returned next to the tensors: `bands` (score std / max |s| / mean largest probability, checked
on the achieved float64 scores by tests/test_attn_regimes_cpu.py) and, for the saturated regime, the winning key of
every row.
"""
import math
import random
from dataclasses import dataclass, field

import torch

from oracle import flashinfer_ref as fr

BF = torch.bfloat16
LOG2E = 1.4426950408889634
WIDE = ["randn", "ints2", "ints4", "ints8", "wide", "mixed"]
STRUCTURED = ["sink", "late-peak", "rising", "falling", "offset"]
REGIMES = WIDE + STRUCTURED                  # + "saturated" (saturated_request)
SM_SCALES = [None, 0.02, 0.25, 1.0]
CALIBRATED_MAXP = (0.3, 0.95)                # sink, late-peak, ramps: mean largest probability per row
SAT_GAP_LOG2 = 160.0                         # exp2(-160) == 0 in fp32 (the smallest subnormal is 2^-149)


@dataclass
class Request:
    q: torch.Tensor              # [n, KH * g, D] bf16
    k: torch.Tensor              # [L, KH, D] bf16 (an fp8 cache: exact byte * k_scale products)
    v: torch.Tensor              # [L, KH, D] bf16
    bands: dict = field(default_factory=dict)
    winner: torch.Tensor = None  # saturated: [n, KH * g] int64, the key whose V row each query row must return


def default_scale(D):
    return 1.0 / math.sqrt(D)


def hadamard(D):
    """Sylvester Hadamard matrix [D, D] of +-1 (D a power of two): pairwise orthogonal rows with exact integer dots."""
    h = torch.ones(1, 1)
    while h.shape[0] < D:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def _limits(n, L, causal):
    return torch.arange(n) + (L - n) if causal else torch.full((n,), L - 1)


def scores_f64(req, sm_scale, causal=True):
    """float64 scores [KH, g, n, L] in nats, masked positions -inf."""
    n, H, D = req.q.shape
    L, KH, _ = req.k.shape
    s = torch.einsum("mhgd,lhd->hgml", req.q.double().view(n, KH, H // KH, D), req.k.double()) * sm_scale
    vis = torch.arange(L).view(1, L) <= _limits(n, L, causal).view(n, 1)
    return s.masked_fill(~vis.view(1, 1, n, L), float("-inf"))


def score_stats(req, sm_scale, causal=True):
    s = scores_f64(req, sm_scale, causal)
    fin = s[torch.isfinite(s)]
    return dict(std=fin.std().item(), max_abs=fin.abs().max().item(), s_max=fin.max().item(),
                span=(fin.max() - fin.min()).item(),
                maxp=torch.softmax(s, -1).amax(-1).mean().item())


def make_request(name, n, L, KH, g, D, seed, sm_scale=None, causal=True):
    """One request of regime `name`: n query tokens x KH * g heads against L keys."""
    sm = default_scale(D) if sm_scale is None else sm_scale
    gen = torch.Generator().manual_seed(seed * 7919 + REGIMES.index(name))
    H = KH * g
    if n == 0 or L == 0:                     # nothing to shape: a request without rows or without keys
        return Request(torch.randn(n, H, D, generator=gen).to(BF), torch.randn(L, KH, D, generator=gen).to(BF),
                       torch.randn(L, KH, D, generator=gen).to(BF))
    rel = sm * math.sqrt(D)                  # score std of randn inputs at this scale
    v = torch.randn(L, KH, D, generator=gen)
    bands = {}
    if name in ("ints2", "ints4", "ints8", "mixed"):
        amp = 2 if name == "mixed" else int(name[4:])
        q = torch.randint(-amp, amp + 1, (n, H, D), generator=gen).float()
        k = torch.randint(-amp, amp + 1, (L, KH, D), generator=gen).float()
        e = amp * (amp + 1) / 3.0            # variance of one entry
        if name == "mixed":
            k[::7] *= 16.0
            k[::5] *= 2.0 ** -12
            bands["std"] = (1.5 * e * rel, 16 * e * rel)
        else:
            bands["std"] = (0.8 * e * rel, 1.25 * e * rel)
    elif name in ("randn", "wide"):
        a, c = (8.0, 4.0) if name == "wide" else (1.0, 1.0)
        q = torch.randn(n, H, D, generator=gen) * a
        k = torch.randn(L, KH, D, generator=gen) * c
        bands["std"] = (0.8 * a * c * rel, 1.25 * a * c * rel)
    else:
        u = hadamard(D)[5]                   # one fixed +-1 direction
        zq = torch.randn(n, H, D, generator=gen)
        zk = torch.randn(L, KH, D, generator=gen)
        zq -= (zq @ u).unsqueeze(-1) * u / D
        zk -= (zk @ u).unsqueeze(-1) * u / D
        comp = 1.0 / rel                     # the same scores at every sm_scale
        a = 4.0
        lim = _limits(n, L, causal)
        shift = torch.zeros(L)               # nats
        if name in ("sink", "late-peak"):
            # half the mass: exp(shift) = sum of the others ~ visible keys * E exp(N(0, 1))
            nvis = float(lim.float().mean()) + 1.0
            shift[0 if name == "sink" else int(lim.min())] = math.log(max(nvis - 1.0, 1.0)) + 0.5
            bands["maxp"] = CALIBRATED_MAXP
        elif name in ("rising", "falling"):
            # nats per key: a span >= 300 from 200 keys on; never so steep that one key takes all the mass
            slope = min(max(300.0 / L, 0.3), 1.5)
            ramp = torch.arange(L).float() * slope
            shift = ramp if name == "rising" else ramp.flip(0)
            bands["maxp"] = CALIBRATED_MAXP
            if L >= 200:
                bands["span"] = (299.0, float("inf"))
        else:                                # offset
            shift[:] = -400.0
            bands["s_max"] = (-440.0, -360.0)
        cvec = shift / (a * math.sqrt(D))    # a * c_i * |u|^2 * sm * comp = a * c_i * sqrt(D)
        q = comp * (zq + a * u)
        k = zk + cvec.view(L, 1, 1) * u
    req = Request(q.to(BF), k.to(BF), v.to(BF), bands)
    if "maxp" in bands:                      # calibrated regimes: at 1.000 the bound test degenerates to 0 / 0
        got = score_stats(req, sm, causal)["maxp"]
        assert bands["maxp"][0] <= got <= bands["maxp"][1], f"{name}: mean largest probability {got:.3f} outside the band"
    return req


def placements(L, n, page_size, causal=True, nsplits=(2, 4, 10)):
    """Key positions where masks, tiles, pages, waves and KV splits begin and end."""
    ntiles = (L + 31) // 32
    pos = [0, 31, 32, 33, page_size - 1, page_size, (L - 1) // page_size * page_size, (L - 1) // page_size * page_size - 1,
           L - 1, L - n, L - n - 1, (ntiles - 1) * 32, (ntiles - 1) * 32 - 1]
    for ns in nsplits:
        tps = (ntiles + ns - 1) // ns
        for s in range(1, ns):
            pos += [s * tps * 32, s * tps * 32 - 1]
    out = []
    for p in pos:
        if 0 <= p < L and p not in out:
            out.append(p)
    return out


def saturated_request(n, L, KH, g, D, seed, sm_scale=None, causal=True, page_size=128, k_scale=None):
    """Every query row has one winning key (see the module docstring).  k_scale [KH] (powers of two) for an fp8 cache:
    K holds e4m3-representable bytes times k_scale[h] and q is scaled by 1 / k_scale[h], so the scores are the same.
    The gap between the winner and every other VISIBLE key is computed in float64 and asserted."""
    sm = default_scale(D) if sm_scale is None else sm_scale
    gen = torch.Generator().manual_seed(seed * 104729 + 17)
    rnd = random.Random(seed)
    H, rows = KH * g, n * g
    had = hadamard(D)
    c = 16.0                                 # winner keys c * u; traps 4 c * t (64: exact in e4m3 and bf16)
    a = 2.0 ** math.ceil(math.log2(400.0 / (c * D * sm * LOG2E)))
    lim = _limits(n, L, causal)
    ntrap = min(n - 1, 16) if causal else 0
    first_trap_tok = n - 1 - ntrap
    free_hi = L - ntrap - 1                  # winners live at or below this key
    q = torch.zeros(n, KH, g, D)
    k = torch.randint(-1, 2, (L, KH, D), generator=gen).float()
    v = torch.randn(L, KH, D, generator=gen)
    winner = torch.zeros(n, KH, g, dtype=torch.int64)
    ndir = min(rows, 32)
    assert free_hi + 1 >= ndir and L - n >= 0, "context too short for one winner per direction"
    for h in range(KH):
        for j in range(ntrap):               # trap of token first_trap_tok + j: one key past its causal limit
            k[int(lim[first_trap_tok + j]) + 1, h] = 4 * c * had[32 + j]
        cand = placements(L, n, page_size, causal)
        cand = cand[(h * len(cand)) // KH + seed % 3:] + cand[:(h * len(cand)) // KH + seed % 3]
        # rows that share a direction share its winner, which all of them must see
        normal = [R for R in range(rows) if not (ntrap and R // g == n - 1)]
        dir_lim = [min([int(lim[R // g]) for R in normal if R % 32 == d], default=-1) for d in range(ndir)]
        used = set()
        wpos = []
        for d in range(ndir):
            top = min(dir_lim[d], free_hi)
            if top < 0:
                wpos.append(-1)
                continue
            p = next((x for x in cand if x <= top and x not in used), None)
            while p is None:
                x = rnd.randint(0, top)
                p = x if x not in used else None
            used.add(p)
            wpos.append(p)
            k[p, h] = c * had[d]
        for R in range(rows):
            i, r = divmod(R, g)
            if ntrap and i == n - 1:         # the last token: the only one that sees key L - 1 (the last trap)
                q[i, h, r] = a * had[32 + ntrap - 1]
                winner[i, h, r] = L - 1
                continue
            q[i, h, r] = a * had[R % 32]
            winner[i, h, r] = wpos[R % 32]
            if i >= first_trap_tok:
                q[i, h, r] += 0.5 * a * had[32 + i - first_trap_tok]
    if k_scale is not None:
        ks = k_scale.float().view(1, KH, 1)
        k = k * ks
        q = q / ks.view(1, KH, 1, 1)
    req = Request(q.view(n, H, D).to(BF), k.to(BF), v.to(BF), {}, winner.view(n, H))
    assert torch.equal(req.q.float(), q.view(n, H, D)) and torch.equal(req.k.float(), k), "inputs must be exact in bf16"
    req.bands["gap_log2"] = (SAT_GAP_LOG2, float("inf"))
    assert saturated_gap_log2(req, sm, causal) >= SAT_GAP_LOG2
    return req


def saturated_gap_log2(req, sm_scale, causal=True):
    """Smallest distance, in log2 units, between a row's winning key and its best other visible key (float64)."""
    s = scores_f64(req, sm_scale, causal) * LOG2E                       # [KH, g, n, L]
    n, H = req.winner.shape
    KH = req.k.shape[1]
    w = req.winner.view(n, KH, H // KH).permute(1, 2, 0).unsqueeze(-1)
    top = s.gather(-1, w)
    assert bool(torch.isfinite(top).all()), "a winning key is masked"
    return (top - s.scatter(-1, w, float("-inf")).amax(-1, keepdim=True)).min().item()


def saturated_expected(req, v_ref=None):
    """[n, H, D] bf16: the V row of every query row's winner (v_ref: the float32 dequantised V of an fp8 cache)."""
    n, H = req.winner.shape
    L, KH, D = req.k.shape
    v = (req.v if v_ref is None else v_ref).float()
    hk = (torch.arange(H) // (H // KH)).view(1, H).expand(n, H)
    return v[req.winner, hk].to(BF)


def rows_equal(a, b, signed_zero=False):
    """Bit-for-bit equality of two bf16 outputs.  signed_zero (fp8 caches only): -0 == +0 -- an fp8 V byte can be -0, and
    an accumulator that starts at +0 returns +0 for it (0 + -0 = +0), the one difference a correct kernel may show."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if signed_zero:
        return not bool(torch.isnan(a.float()).any()) and torch.equal(a.float(), b.float())
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


# ------------------------------------------------------------------------------------------------ paging
def pow2_scales(KH, seed):
    """Per-head fp8 scales: non-monotonic powers of two between 2^-7 and 2^-2."""
    r = random.Random(seed)
    ek = [-7, -2, -5, -3, -6, -4, -2, -7]
    ev = [-3, -6, -2, -7, -4, -5, -7, -2]
    o = r.randrange(8)
    return (torch.tensor([2.0 ** ek[(o + h) % 8] for h in range(KH)]),
            torch.tensor([2.0 ** ev[(o + h) % 8] for h in range(KH)]))


def fit_fp8(reqs, k_scale):
    """Move powers of two from K into q, per kv head, until every K / k_scale fits e4m3's +-448: the scores are the
    same floats, and a wide regime is not flattened by the saturating cast of a 2^-7 scale."""
    for r in reqs:
        L, KH, D = r.k.shape
        n, H, _ = r.q.shape
        if L == 0:
            continue
        k, q = r.k.float(), r.q.float().view(n, KH, H // KH, D)
        for h in range(KH):
            top = k[:, h].abs().max().item() / (fr.FP8_MAX * float(k_scale[h]))
            if top > 1.0:
                f = 2.0 ** math.ceil(math.log2(top))
                k[:, h] /= f
                q[:, h] *= f
        r.k, r.q = k.to(BF), q.view(n, H, D).to(BF)
    return reqs


def build_paged(reqs, page_size=128, seed=0, scatter=True, scales=None, layout="NHD", extra_pages=2):
    """Requests -> a scattered page table.  Unmapped pages and the slots past every request's length hold random finite
    values.  Returns a dict: q, qo, ref_cache (what the float64 reference and the oracle read: the bf16 cache, or the
    float32 byte * scale products of an fp8 one), dev_cache (bf16 / e4m3, in `layout`), indices, indptr, last,
    max_pages, n_max, v_ref (per request: the V rows as the kernel sees them, float32)."""
    g = torch.Generator().manual_seed(1000 + seed)
    L0, KH, D = reqs[0].k.shape
    lens = [r.k.shape[0] for r in reqs]
    B = len(reqs)
    max_pages = max(1, max((l + page_size - 1) // page_size for l in lens))
    tot = B * max_pages + extra_pages
    cache = torch.randn(tot, 2, page_size, KH, D, generator=g).to(BF)
    perm = torch.randperm(tot, generator=g) if scatter else torch.arange(tot)
    indices, indptr, last = [], [0], []
    for b, r in enumerate(reqs):
        npg = (lens[b] + page_size - 1) // page_size
        pages = [int(perm[b * max_pages + i]) for i in range(npg)]
        for i, pg in enumerate(pages):
            lo, hi = i * page_size, min((i + 1) * page_size, lens[b])
            cache[pg, 0, :hi - lo] = r.k[lo:hi]
            cache[pg, 1, :hi - lo] = r.v[lo:hi]
        indices += pages
        indptr.append(indptr[-1] + npg)
        last.append(lens[b] - (npg - 1) * page_size if npg else 0)
    ref_cache = dev_cache = cache
    if scales is not None:
        ks, vs = scales
        c8 = torch.empty(cache.shape, dtype=torch.float8_e4m3fn)
        c8[:, 0] = fr.quantize_fp8(cache[:, 0].reshape(-1, KH, D), ks).view(tot, page_size, KH, D)
        c8[:, 1] = fr.quantize_fp8(cache[:, 1].reshape(-1, KH, D), vs).view(tot, page_size, KH, D)
        ref_cache, dev_cache = fr.dequantize_cache_fp8(c8, ks, vs), c8
    if layout == "HND":
        dev_cache = dev_cache.permute(0, 1, 3, 2, 4).contiguous()
    ns = [r.q.shape[0] for r in reqs]
    qo = torch.tensor([0] + [sum(ns[:i + 1]) for i in range(B)], dtype=torch.int32)
    pt = dict(q=torch.cat([r.q for r in reqs]), qo=qo, ref_cache=ref_cache, dev_cache=dev_cache,
              indices=torch.tensor(indices + [0], dtype=torch.int32), indptr=torch.tensor(indptr, dtype=torch.int32),
              last=torch.tensor(last, dtype=torch.int32), max_pages=max_pages, n_max=max(ns), page_size=page_size,
              layout=layout, scales=scales)
    pt["v_ref"] = [fr.gather_request_kv(ref_cache, pt["indices"], pt["indptr"], pt["last"], b)[1].float() for b in range(B)]
    pt["k_ref"] = [fr.gather_request_kv(ref_cache, pt["indices"], pt["indptr"], pt["last"], b)[0].float() for b in range(B)]
    return pt


# ------------------------------------------------------------------------------------------------ emulation
def emulate_request(q, k, v, KH, sm_scale, causal=True, tile=32, nsplit=1):
    """The kernels' algorithm in plain torch, one request: fp32 scores, log2 domain, online softmax over `tile`-key
    tiles starting from m = -1e30, P rounded to bf16 for the P.V product, fp32 accumulation, `nsplit` contiguous key
    ranges merged with the formula of attn_merge_kernel (M = max m_s; L = sum l_s 2^(m_s - M); O likewise), one division,
    one rounding to bf16.  q [n, H, D], k / v [L, KH, D] (any float dtype: an fp8 cache as its exact float32 values)."""
    n, H, D = q.shape
    L = k.shape[0]
    g = H // KH
    sl2 = torch.tensor(sm_scale * LOG2E, dtype=torch.float32)
    qf = q.float().view(n, KH, g, D).permute(1, 2, 0, 3)                # [KH, g, n, D]
    kf, vf = k.float().permute(1, 0, 2), v.float().permute(1, 0, 2)    # [KH, L, D]
    lim = _limits(n, L, causal).view(1, 1, n, 1)
    ntiles = (L + tile - 1) // tile
    tps = (ntiles + nsplit - 1) // nsplit
    parts = []
    for s_ in range(nsplit):
        m = torch.full((KH, g, n), -1e30, dtype=torch.float32)
        l = torch.zeros(KH, g, n, dtype=torch.float32)
        o = torch.zeros(KH, g, n, D, dtype=torch.float32)
        for t in range(s_ * tps, min(ntiles, (s_ + 1) * tps)):
            lo, hi = t * tile, min(L, (t + 1) * tile)
            sc = torch.einsum("hgnd,hld->hgnl", qf, kf[:, lo:hi]) * sl2
            sc = sc.masked_fill(torch.arange(lo, hi).view(1, 1, 1, -1) > lim, float("-inf"))
            mnew = torch.maximum(m, sc.amax(-1))
            alpha = torch.exp2(m - mnew)
            p = torch.exp2(sc - mnew.unsqueeze(-1))
            l = l * alpha + p.sum(-1)
            o = o * alpha.unsqueeze(-1) + torch.einsum("hgnl,hld->hgnd", p.to(BF).float(), vf[:, lo:hi])
            m = mnew
        parts.append((m, l, o))
    M = torch.stack([p_[0] for p_ in parts]).amax(0)
    Lsum = torch.zeros_like(M)
    acc = torch.zeros_like(parts[0][2])
    for m, l, o in parts:
        sc_ = torch.exp2(m - M)
        Lsum = Lsum + l * sc_
        acc = acc + o * sc_.unsqueeze(-1)
    out = torch.where(Lsum.unsqueeze(-1) > 0, acc / Lsum.unsqueeze(-1).clamp_min(1e-38), torch.zeros_like(acc))
    return out.permute(2, 0, 1, 3).reshape(n, H, D).to(BF)


def emulate_paged(pt, KH, sm_scale, causal=True, nsplit=1):
    outs = []
    for b in range(pt["indptr"].numel() - 1):
        q0, q1 = int(pt["qo"][b]), int(pt["qo"][b + 1])
        outs.append(emulate_request(pt["q"][q0:q1], pt["k_ref"][b], pt["v_ref"][b], KH, sm_scale, causal, nsplit=nsplit))
    return torch.cat(outs)
