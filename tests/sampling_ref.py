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
