// Temperature / top-p sampling and lossless speculative sampling (Leviathan et al. 2023, Chen et al. 2023) for the
// decode loops.  The semantics -- tempered top-p filter, Gumbel-max draw keyed by a counter-based Philox4x32-10
// stream, the verify encoding fed to the unchanged accept kernel -- are stated in include/magicdec_hip.h (K11);
// tests/sampling_ref.py restates them in numpy.
//
// Determinism: every sum is an integer sum (64-bit fixed-point masses added in LDS), every reduction of floats is a
// max / argmax (order-free), so a row's statistics and its draw are bit-identical on every launch and graph replay.
// The iteration counter and the draft-step index live in device memory (counters[0], counters[1]); the last
// workgroup of a launch (ticket counters[2]) advances them, so one captured graph serves every step.
#include "md_common.h"

namespace {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;
constexpr float kMassScale = 1099511627776.0f;  // 2^40

struct Word4 {
    uint32_t x, y, z, w;
};

__host__ __device__ __forceinline__ Word4 philox4x32_10(Word4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += kPhiloxW0;
            k1 += kPhiloxW1;
        }
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c.x;
        const uint64_t p1 = (uint64_t)kPhiloxM1 * c.z;
        Word4 n;
        n.x = (uint32_t)(p1 >> 32) ^ c.y ^ k0;
        n.y = (uint32_t)p1;
        n.z = (uint32_t)(p0 >> 32) ^ c.w ^ k1;
        n.w = (uint32_t)p0;
        c = n;
    }
    return c;
}

struct NoiseKey {
    uint32_t k0, k1;    // seed
    uint32_t req;       // counter word 1: request b
    uint32_t tag;       // counter word 2: purpose << 24 | step
    uint32_t iter;      // counter word 3: iteration counter
};

__device__ __forceinline__ NoiseKey noise_key(uint64_t seed, int purpose, int step, int req, uint32_t iter) {
    NoiseKey k;
    k.k0 = (uint32_t)seed;
    k.k1 = (uint32_t)(seed >> 32);
    k.req = (uint32_t)req;
    k.tag = ((uint32_t)purpose << 24) | ((uint32_t)step & 0xffffffu);
    k.iter = iter;
    return k;
}

// counter word 0 = v >> 2; the uniform of vocab index v is word (v & 3) of that block
__device__ __forceinline__ Word4 noise_block(const NoiseKey& k, int v) {
    return philox4x32_10(Word4{(uint32_t)v >> 2, k.req, k.tag, k.iter}, k.k0, k.k1);
}
__device__ __forceinline__ uint32_t pick(const Word4& w, int v) {
    const int s = v & 3;
    return s == 0 ? w.x : (s == 1 ? w.y : (s == 2 ? w.z : w.w));
}
// (2 (x >> 9) + 1) * 2^-24: exact in fp32, strictly inside (0, 1)
__device__ __forceinline__ float uniform_of(uint32_t x) { return (float)(2u * (x >> 9) + 1u) * 0x1p-24f; }
__device__ __forceinline__ float gumbel_of(uint32_t x) { return -logf(-logf(uniform_of(x))); }

// order-preserving 16-bit key of a bf16 bit pattern (larger key <=> larger value; -0 sorts just below +0)
__device__ __forceinline__ uint32_t key16(uint32_t b) { return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u); }

// the filter's mass of a logit: floor(exp((l - m) * invT) * 2^40) -- <= 2^40, so a 151 936-token row sums below 2^58
__device__ __forceinline__ unsigned long long mass_fx(float l, float m, float invT) {
    return (unsigned long long)(expf((l - m) * invT) * kMassScale);
}

struct RowStats {       // md_sample_stats of the header
    float m;
    uint32_t kstar;
    unsigned long long zkept;
};
static_assert(sizeof(RowStats) == 16, "md_sample_stats is 16 bytes");

// the filtered probability of a logit under a row's stats (the same function for p~ and q~)
__device__ __forceinline__ float prob_of(uint32_t bits, const RowStats& s, float invT) {
    if (key16(bits) < s.kstar) return 0.f;
    return (float)mass_fx(bf16_bits_to_f32(bits), s.m, invT) / (float)s.zkept;
}

struct Smem {
    unsigned long long hist[256];
    float redf[16];
    int redi[16];
    int sel;
    unsigned long long above;
    RowStats st;
    uint32_t iter, step;
    int jr;
};

// f(v, bf16 bits) over one row; 16-byte loads when the row is aligned
template <int NT, class F>
__device__ __forceinline__ void for_row(const unsigned short* __restrict__ row, int vocab, F&& f) {
    int start = 0;
    if ((((uintptr_t)row) & 15) == 0) {
        const int nvec = vocab >> 3;
        for (int i = threadIdx.x; i < nvec; i += NT) {
            const u32x4 raw = reinterpret_cast<const u32x4*>(row)[i];
#pragma unroll
            for (int e = 0; e < 8; ++e) f(i * 8 + e, (raw[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
        }
        start = nvec << 3;
    }
    for (int v = start + threadIdx.x; v < vocab; v += NT) f(v, (uint32_t)row[v]);
}

template <int NT>
__device__ float block_max(float v, Smem& s) {
    v = wave_reduce_max(v);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s.redf[wave] = v;
    __syncthreads();
    float r = s.redf[0];
    for (int w = 1; w < NT / 64; ++w) r = fmaxf(r, s.redf[w]);
    return r;
}

// (score, index) -> the largest score, lowest index among equal ones; -1 if every score is -inf
template <int NT>
__device__ int block_argmax(float best, int bi, Smem& s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > best || (ov == best && oi < bi)) {
            best = ov;
            bi = oi;
        }
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        s.redf[wave] = best;
        s.redi[wave] = bi;
    }
    __syncthreads();
    best = s.redf[0];
    bi = s.redi[0];
    for (int w = 1; w < NT / 64; ++w)
        if (s.redf[w] > best || (s.redf[w] == best && s.redi[w] < bi)) {
            best = s.redf[w];
            bi = s.redi[w];
        }
    return best == -INFINITY ? -1 : bi;
}

// wave 0: sel = min i such that base + sum_{k > i} hist[k] <= thr (exists: i = 255 qualifies whenever base <= thr),
// above = base + sum_{k > sel} hist[k].  Lane l owns bins 4l..4l+3; suffix sums by a fixed-order shuffle scan.
__device__ void scan_select(Smem& s, unsigned long long base, double thr) {
    if (threadIdx.x < 64) {
        const int l = threadIdx.x;
        unsigned long long h[4], own = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            h[e] = s.hist[4 * l + e];
            own += h[e];
        }
        unsigned long long incl = own;  // sum over lanes >= l
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long t = __shfl_down(incl, o);
            if (l + o < 64) incl += t;
        }
        unsigned long long acc = base + (incl - own);  // sum over bins of lanes > l
        int cnt = 0;
        unsigned long long above_here = 0;
        int sel_here = -1;
#pragma unroll
        for (int e = 3; e >= 0; --e) {
            if ((double)acc <= thr) {
                ++cnt;
                sel_here = 4 * l + e;
                above_here = acc;
            }
            acc += h[e];
        }
        // the predicate is monotone in the bin index: the selected bin is the lowest one that passes
        int total = cnt;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o);
        const int sel = 256 - total;
        if (total == 0 && l == 0) {     // unreachable for base <= thr; keeps s.sel defined
            s.sel = 255;
            s.above = base;
        }
        if (sel_here == sel) {
            s.sel = sel;
            s.above = above_here;
        }
    }
    __syncthreads();
}

// m, top-p key threshold and Z_kept of one row (2 passes; 3 when top_p < 1).  Result in s.st.
template <int NT>
__device__ void row_stats(const unsigned short* __restrict__ row, int vocab, float invT, float top_p, Smem& s) {
    float mx = -INFINITY;
    for_row<NT>(row, vocab, [&](int, uint32_t b) { mx = fmaxf(mx, bf16_bits_to_f32(b)); });
    mx = block_max<NT>(mx, s);
    for (int i = threadIdx.x; i < 256; i += NT) s.hist[i] = 0;
    __syncthreads();
    for_row<NT>(row, vocab, [&](int, uint32_t b) {
        const unsigned long long w = mass_fx(bf16_bits_to_f32(b), mx, invT);
        if (w) atomicAdd(&s.hist[key16(b) >> 8], w);
    });
    __syncthreads();
    if (top_p >= 1.f) {
        if (threadIdx.x < 64) {
            unsigned long long z = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) z += s.hist[4 * threadIdx.x + e];
            // fixed-order tree over the lanes
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o);
            if (threadIdx.x == 0) s.st = RowStats{mx, 0u, z};
        }
        __syncthreads();
        return;
    }
    // total Z by a fixed-order tree over the lanes
    if (threadIdx.x < 64) {
        unsigned long long z = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) z += s.hist[4 * threadIdx.x + e];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o);
        if (threadIdx.x == 0) s.above = z;
    }
    __syncthreads();
    const unsigned long long Z = s.above;
    const double thr = (double)top_p * (double)Z;
    __syncthreads();
    scan_select(s, 0ull, thr);
    const int hb = s.sel;
    const unsigned long long above_hb = s.above;
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += NT) s.hist[i] = 0;
    __syncthreads();
    for_row<NT>(row, vocab, [&](int, uint32_t b) {
        const uint32_t k = key16(b);
        if ((int)(k >> 8) == hb) {
            const unsigned long long w = mass_fx(bf16_bits_to_f32(b), mx, invT);
            if (w) atomicAdd(&s.hist[k & 0xffu], w);
        }
    });
    __syncthreads();
    scan_select(s, above_hb, thr);
    if (threadIdx.x == 0) s.st = RowStats{mx, ((uint32_t)hb << 8) | (uint32_t)s.sel, s.above + s.hist[s.sel]};
    __syncthreads();
}

// Gumbel-max over the kept tokens of a row: argmax of (l - m) * invT + G(v); optionally copies the row to `copy_to`
template <int NT>
__device__ int draw_row(const unsigned short* __restrict__ row, int vocab, const RowStats& st, float invT,
                        const NoiseKey& nk, Smem& s, unsigned short* __restrict__ copy_to) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    int grp = -1;
    Word4 w{0, 0, 0, 0};
    auto visit = [&](int v, uint32_t b) {
        if (key16(b) < st.kstar) return;
        if ((v >> 2) != grp) {
            grp = v >> 2;
            w = noise_block(nk, v);
        }
        const float sc = (bf16_bits_to_f32(b) - st.m) * invT + gumbel_of(pick(w, v));
        if (sc > best || (sc == best && v < bi)) {
            best = sc;
            bi = v;
        }
    };
    int start = 0;
    if (((((uintptr_t)row) | (uintptr_t)copy_to) & 15) == 0) {
        const int nvec = vocab >> 3;
        for (int i = threadIdx.x; i < nvec; i += NT) {
            const u32x4 raw = reinterpret_cast<const u32x4*>(row)[i];
            if (copy_to) reinterpret_cast<u32x4*>(copy_to)[i] = raw;
#pragma unroll
            for (int e = 0; e < 8; ++e) visit(i * 8 + e, (raw[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
        }
        start = nvec << 3;
    }
    for (int v = start + threadIdx.x; v < vocab; v += NT) {
        const unsigned short b = row[v];
        if (copy_to) copy_to[v] = b;
        visit(v, (uint32_t)b);
    }
    const int t = block_argmax<NT>(best, bi, s);
    return t < 0 ? 0 : t;
}

// last workgroup of the launch advances the counters: ADVANCE_STEP -> step += 1; ADVANCE_ITER -> iter += 1, step = 0
__device__ void ticket_advance(int32_t* counters, int advance) {
    __syncthreads();
    if (threadIdx.x == 0 && advance != MD_SAMPLE_ADVANCE_NONE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const int t = __hip_atomic_fetch_add(&counters[2], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (t == (int)gridDim.x - 1) {
            __hip_atomic_exchange(&counters[2], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (advance == MD_SAMPLE_ADVANCE_STEP) {
                __hip_atomic_fetch_add(&counters[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                __hip_atomic_fetch_add(&counters[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_exchange(&counters[1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

__device__ void read_counters(const int32_t* counters, Smem& s) {
    if (threadIdx.x == 0) {
        s.iter = (uint32_t)__hip_atomic_load(&counters[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s.step = (uint32_t)__hip_atomic_load(&counters[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
}

struct SampleParams {
    const unsigned short* logits;
    int64_t row_stride;
    int n, vocab, purpose, advance, gamma;
    float invT, top_p;
    uint64_t seed;
    const int64_t* row_sel;
    int32_t* counters;
    unsigned short* ring;   // [B, gamma, vocab] or null
    RowStats* ring_stats;   // [B, gamma] or null
    int64_t* out;           // [B, n]
};

// one workgroup per request: stats + draw of ONE row (row_sel[b] - 1, else the last), token to all n columns
template <int NT>
__global__ __launch_bounds__(NT) void sample_rows_kernel(const SampleParams p) {
    __shared__ Smem s;
    const int b = blockIdx.x;
    read_counters(p.counters, s);
    int r = p.n - 1;
    if (p.row_sel) {
        const int64_t q = p.row_sel[b] - 1;
        r = q < 0 ? 0 : (q >= p.n ? p.n - 1 : (int)q);
    }
    const unsigned short* row = p.logits + ((int64_t)b * p.n + r) * p.row_stride;
    row_stats<NT>(row, p.vocab, p.invT, p.top_p, s);
    const RowStats st = s.st;
    const bool draft = p.ring != nullptr;
    const int j = draft ? (int)s.step : 0;
    const bool store = draft && j >= 0 && j < p.gamma;
    unsigned short* copy_to = store ? p.ring + ((int64_t)b * p.gamma + j) * p.vocab : nullptr;
    const NoiseKey nk = noise_key(p.seed, p.purpose, j, b, s.iter);
    const int tok = draw_row<NT>(row, p.vocab, st, p.invT, nk, s, copy_to);
    if (threadIdx.x == 0) {
        for (int c = 0; c < p.n; ++c) p.out[(int64_t)b * p.n + c] = tok;
        if (store) p.ring_stats[(int64_t)b * p.gamma + j] = st;
    }
    ticket_advance(p.counters, p.advance);
}

// stats of every target row of a verify step (one workgroup per row)
template <int NT>
__global__ __launch_bounds__(NT) void row_stats_kernel(const unsigned short* __restrict__ logits, int64_t row_stride,
                                                       int vocab, float invT, float top_p, RowStats* out) {
    __shared__ Smem s;
    row_stats<NT>(logits + (int64_t)blockIdx.x * row_stride, vocab, invT, top_p, s);
    if (threadIdx.x == 0) out[blockIdx.x] = s.st;
}

struct VerifyParams {
    const unsigned short* logits;  // [B*(gamma+1), row_stride]
    int64_t row_stride;
    int gamma, vocab;
    float invT;
    uint64_t seed;
    const int64_t* tokens_buffer;   // [B, gamma+1]
    const unsigned short* ring;     // [B, gamma, vocab]
    const RowStats* ring_stats;     // [B, gamma]
    const RowStats* target_stats;   // [B*(gamma+1)]
    int32_t* counters;
    int64_t* target_tokens;         // [B, gamma+1]
};

// Speculative verify of request b, written as the target_tokens the unchanged accept kernel (csrc/accept.hip) reads:
//   target_tokens[b, j] = d_j (= tokens_buffer[b, j+1]) for every accepted position j < jr,
//   target_tokens[b, jr] = the corrected token (residual sample at the first rejection jr, or the bonus if jr = gamma),
//   target_tokens[b, j > jr] = -1 (never read: the accept loop stops at jr).
// Why md_accept_rollback then computes the speculative-sampling outcome: its `tt[j] == d` test holds exactly at the
// accepted positions.  At the rejected position jr, u q~(d) >= p~(d) with u < 1, so p~(d) < q~(d) (or both are 0): the
// residual max(p~ - q~, 0) is 0 at d and its sample is never d.  (If the residual rounds to zero everywhere the token is
// drawn from p~ with d excluded, for the same reason.)  So its accept count is jr + 1 -- cut at an EOT draft token
// exactly as in the greedy loop -- and its bonus tt[an - 1] is the corrected token.
template <int NT>
__global__ __launch_bounds__(NT) void spec_verify_kernel(const VerifyParams p) {
    __shared__ Smem s;
    const int b = blockIdx.x, G = p.gamma;
    read_counters(p.counters, s);
    const uint32_t iter = s.iter;
    const int64_t* tb = p.tokens_buffer + (int64_t)b * (G + 1);
    auto trow = [&](int j) { return p.logits + ((int64_t)b * (G + 1) + j) * p.row_stride; };
    auto rrow = [&](int j) { return p.ring + ((int64_t)b * G + j) * p.vocab; };
    if (threadIdx.x == 0) {
        int jr = G;
        for (int j = 0; j < G; ++j) {
            const int64_t d = tb[j + 1];
            if (d < 0 || d >= p.vocab) {
                jr = j;
                break;
            }
            const float pd = prob_of(trow(j)[d], p.target_stats[(int64_t)b * (G + 1) + j], p.invT);
            const float qd = prob_of(rrow(j)[d], p.ring_stats[(int64_t)b * G + j], p.invT);
            const NoiseKey nk = noise_key(p.seed, MD_SAMPLE_ACCEPT, j, b, iter);
            const float u = uniform_of(noise_block(nk, 0).x);
            if (!(u * qd < pd)) {
                jr = j;
                break;
            }
        }
        s.jr = jr;
    }
    __syncthreads();
    const int jr = s.jr;
    int tok;
    if (jr < G) {
        const RowStats ps = p.target_stats[(int64_t)b * (G + 1) + jr];
        const RowStats qs = p.ring_stats[(int64_t)b * G + jr];
        const int64_t d = tb[jr + 1];
        const unsigned short* tr = trow(jr);
        const unsigned short* rr = rrow(jr);
        const NoiseKey nk = noise_key(p.seed, MD_SAMPLE_RESIDUAL, jr, b, iter);
        float best = -INFINITY;
        int bi = 0x7fffffff, grp = -1;
        Word4 w{0, 0, 0, 0};
        for (int v = threadIdx.x; v < p.vocab; v += NT) {
            const float r = prob_of(tr[v], ps, p.invT) - prob_of(rr[v], qs, p.invT);
            if (!(r > 0.f)) continue;
            if ((v >> 2) != grp) {
                grp = v >> 2;
                w = noise_block(nk, v);
            }
            const float sc = logf(r) + gumbel_of(pick(w, v));
            if (sc > best || (sc == best && v < bi)) {
                best = sc;
                bi = v;
            }
        }
        tok = block_argmax<NT>(best, bi, s);
        if (tok < 0) {
            // the residual rounded to zero everywhere: draw from p~ (without the rejected d, which the accept kernel
            // would otherwise read as an acceptance)
            best = -INFINITY;
            bi = 0x7fffffff;
            grp = -1;
            for (int v = threadIdx.x; v < p.vocab; v += NT) {
                const uint32_t bits = tr[v];
                if (v == d || key16(bits) < ps.kstar) continue;
                if ((v >> 2) != grp) {
                    grp = v >> 2;
                    w = noise_block(nk, v);
                }
                const float sc = (bf16_bits_to_f32(bits) - ps.m) * p.invT + gumbel_of(pick(w, v));
                if (sc > best || (sc == best && v < bi)) {
                    best = sc;
                    bi = v;
                }
            }
            tok = block_argmax<NT>(best, bi, s);
            if (tok < 0) tok = d == 0 ? 1 : 0;
        }
    } else {
        const NoiseKey nk = noise_key(p.seed, MD_SAMPLE_BONUS, G, b, iter);
        tok = draw_row<NT>(trow(G), p.vocab, p.target_stats[(int64_t)b * (G + 1) + G], p.invT, nk, s, nullptr);
    }
    if (threadIdx.x == 0) {
        int64_t* tt = p.target_tokens + (int64_t)b * (G + 1);
        for (int j = 0; j <= G; ++j) tt[j] = j < jr ? tb[j + 1] : (j == jr ? (int64_t)tok : (int64_t)-1);
    }
    ticket_advance(p.counters, MD_SAMPLE_ADVANCE_ITER);
}

bool wide(int rows, int vocab) { return rows <= 512 && vocab >= 16384; }

}  // namespace

extern "C" int md_philox4x32_10_host(const uint32_t* ctr_host, int n, uint32_t key0, uint32_t key1,
                                     uint32_t* out_host) {
    MD_CHECK_ARG(ctr_host && out_host && n > 0, "md_philox4x32_10_host: bad arguments");
    for (int i = 0; i < n; ++i) {
        const Word4 c{ctr_host[4 * i], ctr_host[4 * i + 1], ctr_host[4 * i + 2], ctr_host[4 * i + 3]};
        const Word4 r = philox4x32_10(c, key0, key1);
        out_host[4 * i] = r.x;
        out_host[4 * i + 1] = r.y;
        out_host[4 * i + 2] = r.z;
        out_host[4 * i + 3] = r.w;
    }
    return MD_OK;
}

extern "C" int md_sample_rows(const void* logits, int64_t row_stride, int B, int n, int vocab, float temperature,
                              float top_p, uint64_t seed, int purpose, const int64_t* row_sel, int32_t* counters,
                              int advance, void* ring, void* ring_stats, int gamma, int64_t* tokens_out,
                              md_stream_t stream) {
    MD_CHECK_ARG(logits && counters && tokens_out, "md_sample_rows: null pointer argument");
    MD_CHECK_ARG(B > 0 && n > 0 && vocab > 0 && row_stride >= 0, "md_sample_rows: bad shape B=%d n=%d vocab=%d", B, n,
                 vocab);
    MD_CHECK_ARG(temperature > 0.f && top_p > 0.f && top_p <= 1.f,
                 "md_sample_rows: need temperature > 0 and 0 < top_p <= 1 (got %g, %g)", temperature, top_p);
    MD_CHECK_ARG(purpose >= 0 && purpose <= MD_SAMPLE_BONUS, "md_sample_rows: bad purpose %d", purpose);
    MD_CHECK_ARG(advance >= MD_SAMPLE_ADVANCE_NONE && advance <= MD_SAMPLE_ADVANCE_ITER,
                 "md_sample_rows: bad advance mode %d", advance);
    MD_CHECK_ARG((ring == nullptr) == (ring_stats == nullptr), "md_sample_rows: ring and ring_stats go together");
    MD_CHECK_ARG(ring == nullptr || gamma >= 1, "md_sample_rows: a draft ring needs gamma >= 1");
    SampleParams p;
    p.logits = (const unsigned short*)logits;
    p.row_stride = row_stride;
    p.n = n;
    p.vocab = vocab;
    p.purpose = purpose;
    p.advance = advance;
    p.gamma = gamma;
    p.invT = 1.0f / temperature;
    p.top_p = top_p;
    p.seed = seed;
    p.row_sel = row_sel;
    p.counters = counters;
    p.ring = (unsigned short*)ring;
    p.ring_stats = (RowStats*)ring_stats;
    p.out = tokens_out;
    if (wide(B, vocab))
        hipLaunchKernelGGL((sample_rows_kernel<1024>), dim3(B), dim3(1024), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL((sample_rows_kernel<256>), dim3(B), dim3(256), 0, (hipStream_t)stream, p);
    MD_CHECK_LAUNCH("md_sample_rows");
    return MD_OK;
}

extern "C" int md_spec_verify_sample(const void* logits, int64_t row_stride, int B, int gamma, int vocab,
                                     float temperature, float top_p, uint64_t seed, const int64_t* tokens_buffer,
                                     const void* ring, const void* ring_stats, void* target_stats, int32_t* counters,
                                     int64_t* target_tokens, md_stream_t stream) {
    MD_CHECK_ARG(logits && tokens_buffer && ring && ring_stats && target_stats && counters && target_tokens,
                 "md_spec_verify_sample: null pointer argument");
    MD_CHECK_ARG(B > 0 && gamma >= 1 && vocab > 0 && row_stride >= vocab,
                 "md_spec_verify_sample: bad shape B=%d gamma=%d vocab=%d", B, gamma, vocab);
    MD_CHECK_ARG(temperature > 0.f && top_p > 0.f && top_p <= 1.f,
                 "md_spec_verify_sample: need temperature > 0 and 0 < top_p <= 1 (got %g, %g)", temperature, top_p);
    const float invT = 1.0f / temperature;
    const int rows = B * (gamma + 1);
    if (wide(rows, vocab))
        hipLaunchKernelGGL((row_stats_kernel<1024>), dim3(rows), dim3(1024), 0, (hipStream_t)stream,
                           (const unsigned short*)logits, row_stride, vocab, invT, top_p, (RowStats*)target_stats);
    else
        hipLaunchKernelGGL((row_stats_kernel<256>), dim3(rows), dim3(256), 0, (hipStream_t)stream,
                           (const unsigned short*)logits, row_stride, vocab, invT, top_p, (RowStats*)target_stats);
    MD_CHECK_LAUNCH("md_spec_verify_sample(stats)");
    VerifyParams p;
    p.logits = (const unsigned short*)logits;
    p.row_stride = row_stride;
    p.gamma = gamma;
    p.vocab = vocab;
    p.invT = invT;
    p.seed = seed;
    p.tokens_buffer = tokens_buffer;
    p.ring = (const unsigned short*)ring;
    p.ring_stats = (const RowStats*)ring_stats;
    p.target_stats = (const RowStats*)target_stats;
    p.counters = counters;
    p.target_tokens = target_tokens;
    if (wide(B, vocab))
        hipLaunchKernelGGL((spec_verify_kernel<1024>), dim3(B), dim3(1024), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL((spec_verify_kernel<256>), dim3(B), dim3(256), 0, (hipStream_t)stream, p);
    MD_CHECK_LAUNCH("md_spec_verify_sample");
    return MD_OK;
}
