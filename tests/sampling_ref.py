"""numpy restatement of the sampling semantics of include/magicdec_hip.h (K11) -- helper of the sampling tests.

Philox4x32-10 and the noise layout are restated bit for bit (uint32 arithmetic); the filter, the probabilities and the
draws are computed in float64 and report how close each decision came to flipping, so that a test can tell a kernel
defect from a decision the kernel's fp32 arithmetic may legitimately take the other way (`margin < TOL`)."""
from __future__ import annotations

import numpy as np

PREFILL, BASELINE, DRAFT, ACCEPT, RESIDUAL, BONUS = range(6)
TOL = 1e-5
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(ctr, k0, k1):
    """ctr: uint32 [n, 4] -> uint32 [n, 4] (Random123's philox4x32 with 10 rounds)."""
    c = np.asarray(ctr, dtype=np.uint64).reshape(-1, 4).copy()
    k0, k1 = np.uint64(k0 & _MASK), np.uint64(k1 & _MASK)
    mask = np.uint64(_MASK)
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(_W0)) & mask
            k1 = (k1 + np.uint64(_W1)) & mask
        p0 = np.uint64(_M0) * c[:, 0]
        p1 = np.uint64(_M1) * c[:, 2]
        c = np.stack([((p1 >> np.uint64(32)) ^ c[:, 1] ^ k0) & mask, p1 & mask,
                      ((p0 >> np.uint64(32)) ^ c[:, 3] ^ k1) & mask, p0 & mask], axis=1)
    return c.astype(np.uint32)


def words(seed, purpose, step, req, iteration, v):
    """The noise word of vocab indices v (array) of (seed, purpose, step, request, iteration)."""
    v = np.asarray(v, dtype=np.int64)
    ctr = np.zeros((v.size, 4), dtype=np.uint64)
    ctr[:, 0] = v >> 2
    ctr[:, 1] = req & _MASK
    ctr[:, 2] = ((purpose << 24) | (step & 0xFFFFFF)) & _MASK
    ctr[:, 3] = iteration & _MASK
    out = philox4x32_10(ctr, seed & _MASK, (seed >> 32) & _MASK)
    return out[np.arange(v.size), v & 3]


def uniforms(w):
    """(2 (x >> 9) + 1) * 2^-24 (exact in fp32 and float64)."""
    return ((2 * (np.asarray(w, dtype=np.uint64) >> np.uint64(9)) + 1).astype(np.float64)) * 2.0 ** -24


def gumbel(u):
    return -np.log(-np.log(u))


def bf16_bits(x):
    """float32 array -> bf16 bit patterns (round to nearest even) as uint16."""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    return b.astype(np.uint16)


def bits_to_f(bits):
    return (np.asarray(bits, dtype=np.uint32) << 16).view(np.float32).astype(np.float64)


def key16(bits):
    b = np.asarray(bits, dtype=np.uint32)
    return np.where(b & 0x8000, (~b) & 0xFFFF, b | 0x8000)


def inv_t(T):
    return float(np.float32(1.0) / np.float32(T))


def row_filter(bits, T, top_p):
    """-> dict(m, kstar, keep [V] bool, w [V] float64 masses exp((l-m) invT), zkept, margin): the tempered top-p filter
    with the tie rule.  margin = relative distance of the top-p mass test from its boundary (tiny = may flip)."""
    l = bits_to_f(bits)
    m = l.max()
    w = np.exp((l - m) * inv_t(T))
    k = key16(bits)
    Z = w.sum()
    if top_p >= 1:
        return dict(m=m, kstar=0, keep=np.ones(len(l), bool), w=w, zkept=Z, margin=np.inf)
    # mass of strictly larger keys, per distinct key
    uk, inv = np.unique(k, return_inverse=True)
    mass_k = np.bincount(inv, weights=w, minlength=len(uk))
    above = np.cumsum(mass_k[::-1])[::-1] - mass_k          # sum over keys > uk[i]
    thr = top_p * Z
    ok = above <= thr
    kstar = int(uk[ok].min())
    keep = k >= kstar
    margin = float(np.min(np.abs(above - thr)) / Z)
    return dict(m=m, kstar=kstar, keep=keep, w=w, zkept=w[keep].sum(), margin=margin)


def probs(f):
    return np.where(f["keep"], f["w"] / f["zkept"], 0.0)


def gumbel_argmax(scores):
    """argmax (lowest index on ties) and the relative gap to the runner-up."""
    i = int(np.argmax(scores))
    s = np.sort(scores[np.isfinite(scores)])
    gap = (s[-1] - s[-2]) / max(1.0, abs(s[-1])) if len(s) > 1 else np.inf
    return i, gap


def draw(bits, T, top_p, seed, purpose, step, req, iteration):
    """-> (token, filter dict, flagged): Gumbel-max over the kept tokens of one row."""
    f = row_filter(bits, T, top_p)
    V = len(bits)
    g = gumbel(uniforms(words(seed, purpose, step, req, iteration, np.arange(V))))
    sc = np.where(f["keep"], (bits_to_f(bits) - f["m"]) * inv_t(T) + g, -np.inf)
    tok, gap = gumbel_argmax(sc)
    return tok, f, bool(gap < TOL or f["margin"] < TOL)


def verify(tbits, rbits, tokens, T, top_p, seed, req, iteration):
    """Speculative verify of one request: tbits [gamma+1, V] target rows, rbits [gamma, V] draft ring rows, tokens
    [gamma+1] the tokens_buffer row -> (target_tokens [gamma+1], flagged)."""
    G = len(tokens) - 1
    V = tbits.shape[1]
    flagged = False
    out = np.full(G + 1, -1, dtype=np.int64)
    for j in range(G):
        d = int(tokens[j + 1])
        fp, fq = row_filter(tbits[j], T, top_p), row_filter(rbits[j], T, top_p)
        flagged |= fp["margin"] < TOL or fq["margin"] < TOL
        p, q = probs(fp), probs(fq)
        u = uniforms(words(seed, ACCEPT, j, req, iteration, [0]))[0]
        lhs, rhs = u * q[d], p[d]
        flagged |= abs(lhs - rhs) < TOL * max(rhs, 1e-30)
        if lhs < rhs:
            out[j] = d
            continue
        r = np.maximum(p - q, 0.0)
        g = gumbel(uniforms(words(seed, RESIDUAL, j, req, iteration, np.arange(V))))
        small = r <= TOL * max(p.max(), q.max())
        flagged |= bool(np.any(small & (r > 0)))
        if np.any(r > 0):
            sc = np.where(r > 0, np.log(np.where(r > 0, r, 1.0)) + g, -np.inf)
        else:
            sc = np.where(fp["keep"] & (np.arange(V) != d), (bits_to_f(tbits[j]) - fp["m"]) * inv_t(T) + g, -np.inf)
        tok, gap = gumbel_argmax(sc)
        flagged |= gap < TOL
        out[j] = tok
        return out, flagged
    tok, f, fl = draw(tbits[G], T, top_p, seed, BONUS, G, req, iteration)
    out[G] = tok
    return out, flagged or fl


def textbook_verify(p_rows, q_rows, drafts, us, residual_token):
    """The textbook algorithm (Leviathan et al. 2023, Algorithm 1) for one request: accept draft j iff
    u_j < p_j(d)/q_j(d); at the first rejection emit residual_token(j) -> (accept count, corrected token or None)."""
    for j, d in enumerate(drafts):
        if us[j] < min(1.0, p_rows[j][d] / q_rows[j][d]):
            continue
        return j, residual_token(j)
    return len(drafts), None


# ------------------------------------------------------------------------------------ the admissible-outcome oracle
# draw / verify above answer "what does float64 arithmetic decide, and was it close?".  On a real vocabulary some
# decision of nearly every request is close by their measure, so the functions below answer a sharper question: given
# the row statistics the kernel itself wrote (checked first, by check_stats), which outcomes can the kernel's fp32
# operation chain reach?  A test then asserts membership in that set; the set is a single outcome almost always.
#
# REL: relative error of the kernel's p~(v) = fp32(w_v) / fp32(zkept) against exp(x_v) 2^40 / zkept evaluated in
# float64, beyond the floor.  In mass_fx / prob_of, x_v = fp32(fp32(l_v - m) * invT) is IEEE fp32 arithmetic without a
# contraction opportunity (a subtraction feeding a multiplication whose product goes to expf), so numpy's float32
# reproduces it bit for bit and it carries no error at all (the draws' scores add G to the product and may be contracted:
# see draw_admissible).  What is left, in units of 2^-24 (half an fp32 ulp, the bound of one correctly rounded operation):
#   expf          HIP documents 1 ulp for expf, i.e. <= 2 units; we allow 2 ulp = 4 units,
#   (float) w_v   one rounding of the uint64 -> fp32 conversion: 1 unit (w_v <= 2^40 > 2^24),
#   (float) zkept one rounding: 1 unit,
#   the divide    correctly rounded (hipcc's default for fp32 division): 1 unit,
# 7 units to first order; 8 units = 2^-21 covers the second-order products.  The floor in w_v adds one unit of the fixed
# point, 1 / zkept in probability (zkept the integer), and p~ is exactly 0 outside the kept set (an integer key compare).
REL = 2.0 ** -21
SUB = 2.0 ** -24         # one fp32 rounding (the residual's subtraction, the accept test's product)


def noise_row(seed, purpose, step, req, iteration, V):
    """The V noise words of a row: words(...) for v = 0..V-1, one Philox block per four tokens."""
    nb = (V + 3) // 4
    ctr = np.zeros((nb, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(nb)
    ctr[:, 1] = req & _MASK
    ctr[:, 2] = ((purpose << 24) | (step & 0xFFFFFF)) & _MASK
    ctr[:, 3] = iteration & _MASK
    return philox4x32_10(ctr, seed & _MASK, (seed >> 32) & _MASK).reshape(-1)[:V]


def _f32(bits):
    return (np.asarray(bits, dtype=np.uint32) << 16).view(np.float32)


def exponents(bits, m, T):
    """x_v = fp32(fp32(l_v - m) * invT), the kernel's own fp32 values, widened to float64."""
    with np.errstate(invalid="ignore"):
        return ((_f32(bits) - np.float32(m)) * np.float32(inv_t(T))).astype(np.float64)


def _select(k, w, top_p):
    """-> (kstar of the float64 masses w, the set of keys the kernel may report): the smallest key whose strictly larger
    keys carry <= fp32(top_p) Z; when that test is within TOL Z of its boundary at kstar (or at the distinct key just
    below it) the neighbouring distinct key on that side is allowed as well."""
    mass = np.bincount(k, weights=w, minlength=65536)
    uk = np.nonzero(np.bincount(k, minlength=65536))[0]
    mk = mass[uk]
    above = np.cumsum(mk[::-1])[::-1] - mk
    Z = float(mk.sum())
    thr = float(np.float32(top_p)) * Z
    i0 = int(np.argmax(above <= thr))              # above is non-increasing in the key and 0 at the largest key
    allowed = {int(uk[i0])}
    if i0 + 1 < len(uk) and abs(above[i0] - thr) < TOL * Z:
        allowed.add(int(uk[i0 + 1]))
    if i0 > 0 and abs(above[i0 - 1] - thr) < TOL * Z:
        allowed.add(int(uk[i0 - 1]))
    return int(uk[i0]), allowed


class Row:
    """One logits row under given statistics (m, kstar, integer zkept): everything downstream of the stats."""

    def __init__(self, bits, T, m, kstar, zkept):
        self.bits = np.asarray(bits, dtype=np.uint16)
        self.T, self.m, self.kstar, self.zkept = T, np.float32(m), int(kstar), int(zkept)
        self.x = exponents(self.bits, self.m, T)
        self.keep = key16(self.bits) >= self.kstar
        self.p = np.where(self.keep, np.exp(self.x) * 2.0 ** 40 / self.zkept, 0.0)
        self.err = np.where(self.keep, 1.0 / self.zkept + REL * self.p, 0.0)

    def same_function(self, other):
        return self.m == other.m and self.kstar == other.kstar and self.zkept == other.zkept and self.T == other.T


def ref_stats(bits, T, top_p):
    """The restatement's own (m, kstar, zkept): float64 selection, integer sum of the floored float64 masses."""
    m = _f32(bits).max()
    w = np.exp(exponents(bits, m, T))
    kstar = 0 if top_p >= 1 else _select(key16(bits), w, top_p)[0]
    wi = np.floor(w * 2.0 ** 40).astype(np.int64)
    return np.float32(m), kstar, int(wi[key16(bits) >= kstar].sum())


def ref_row(bits, T, top_p):
    return Row(bits, T, *ref_stats(bits, T, top_p))


def check_stats(bits, T, top_p, m, kstar, zkept, tag=""):
    """Assert the statistics a kernel wrote for a row and return the Row conditioned on them: m exactly; kstar equal to
    the float64 selection's (or its neighbour on the side of a boundary margin < TOL, nothing else); zkept within 1e-5
    of the float64 sum for THAT kstar."""
    bits = np.asarray(bits, dtype=np.uint16)
    m_ref = _f32(bits).max()
    assert np.float32(m) == m_ref, f"{tag}: m {m} != {m_ref}"
    w = np.exp(exponents(bits, m_ref, T))
    k = key16(bits)
    if top_p >= 1:
        assert int(kstar) == 0, f"{tag}: kstar {kstar} with top_p = 1"
    else:
        ref, allowed = _select(k, w, top_p)
        assert int(kstar) in allowed, f"{tag}: kstar {int(kstar):#x}, restatement {ref:#x} (allowed {sorted(allowed)})"
    zsum = float(w[k >= int(kstar)].sum())
    assert abs(float(zkept) / 2.0 ** 40 - zsum) <= 1e-5 * zsum, f"{tag}: zkept {zkept} vs {zsum * 2.0 ** 40}"
    return Row(bits, T, m, kstar, zkept)


def _slack(s, widen):
    return widen * TOL * np.maximum(1.0, np.abs(np.where(np.isfinite(s), s, 0.0)))


def draw_admissible(row, seed, purpose, step, req, iteration, exclude=None, widen=1.0):
    """Plain Gumbel-max draw over the kept tokens of `row` (draft, prefill, baseline, bonus; with `exclude` the
    fallback draw from p~ without d) -> sorted array of the tokens whose score is within the logf / Gumbel slack
    TOL max(1, |s|) of the best one.  The kernel's score (l - m) * invT + G is NOT bit-equal to row.x + g: besides the
    two logf of G, the compiler may contract the multiply and the add into one fma (one rounding instead of two, a
    difference of <= 2^-24 |x|); the same slack absorbs that.  widen = 0 gives the float64 decision alone."""
    V = len(row.bits)
    g = gumbel(uniforms(noise_row(seed, purpose, step, req, iteration, V)))
    s = np.where(row.keep, row.x + g, -np.inf)
    if exclude is not None and 0 <= exclude < V:
        s[exclude] = -np.inf
    if not np.isfinite(s).any():                       # nothing to draw from: the kernels' documented stand-ins
        return np.array([1 if exclude == 0 else 0])
    sl = _slack(s, widen)
    return np.nonzero(s + sl >= (s - sl).max())[0]


def residual_admissible(P, Q, d, seed, step, req, iteration, widen=1.0):
    """The corrected token at a rejection: Gumbel-max over log max(p~ - q~, 0).  r_v = p~ - q~ is known to
    err_v = err_p + err_q + one rounding of the subtraction; where both rows are the same function of the same bits
    (equal stats, equal logit) r_v is exactly 0.  Token t is admissible iff its upper-bound score log(r + err) + G
    reaches the best lower-bound score log(r - err) + G (-inf where r - err <= 0).  If no token has r - err > 0 the
    kernel may find the residual zero everywhere: then the draw from p~ without d (same noise key) is admissible too,
    and it is the only branch when no token has r + err > 0."""
    V = len(P.bits)
    r = P.p - Q.p
    err = widen * (P.err + Q.err + SUB * np.abs(r))
    if P.same_function(Q):
        exact = P.bits == Q.bits
        r = np.where(exact, 0.0, r)
        err = np.where(exact, 0.0, err)
    up, lo = r + err, r - err
    out = []
    if (up > 0).any():
        g = gumbel(uniforms(noise_row(seed, RESIDUAL, step, req, iteration, V)))
        with np.errstate(divide="ignore", invalid="ignore"):
            hi_s = np.where(up > 0, np.log(np.where(up > 0, up, 1.0)) + g, -np.inf)
            lo_s = np.where(lo > 0, np.log(np.where(lo > 0, lo, 1.0)) + g, -np.inf)
        out.append(np.nonzero(hi_s + _slack(hi_s, widen) >= (lo_s - _slack(lo_s, widen)).max())[0])
        out[0] = out[0][up[out[0]] > 0]
    if not (lo > 0).any():
        out.append(draw_admissible(P, seed, RESIDUAL, step, req, iteration, exclude=d, widen=widen))
    return np.unique(np.concatenate(out))


def verify_admissible(trows, rrows, tokens, seed, req, iteration, widen=1.0):
    """Speculative verify of one request under the kernel's statistics: trows = the gamma+1 target Rows, rrows = the
    gamma ring Rows, tokens = the tokens_buffer row -> list of the admissible target_tokens rows (int64 arrays),
    following every admissible branch.  A draft token outside [0, vocab) is a rejection at its position.  The accept
    test u q~(d) < p~(d) may go either way only when |u q~(d) - p~(d)| is inside err_p + u err_q + one rounding of the
    product."""
    G, V = len(rrows), len(trows[0].bits)
    outs, prefix = [], []
    for j in range(G):
        d = int(tokens[j + 1])
        P, Q = trows[j], rrows[j]
        if 0 <= d < V:
            u = float(uniforms(words(seed, ACCEPT, j, req, iteration, [0]))[0])
            exact = P.same_function(Q) and P.bits[d] == Q.bits[d]
            gap = u * Q.p[d] - P.p[d]
            bound = widen * ((0.0 if exact else P.err[d] + u * Q.err[d]) + SUB * u * Q.p[d])
            can_acc, can_rej = gap < bound, gap >= -bound
            if bound == 0:
                can_acc, can_rej = gap < 0, gap >= 0
        else:
            can_acc, can_rej = False, True
        if can_rej:
            for t in residual_admissible(P, Q, d, seed, j, req, iteration, widen):
                outs.append(np.array(prefix + [int(t)] + [-1] * (G - j), dtype=np.int64))
        if not can_acc:
            return outs
        prefix.append(d)
    for t in draw_admissible(trows[G], seed, BONUS, G, req, iteration, widen=widen):
        outs.append(np.array(prefix + [int(t)], dtype=np.int64))
    return outs


def contains(rows, row):
    return any(np.array_equal(r, row) for r in rows)
