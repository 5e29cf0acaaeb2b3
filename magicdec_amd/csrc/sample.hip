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

// for_row that also copies the row to `copy_to` (may be null); 16-byte loads and stores when both are aligned
template <int NT, class F>
__device__ __forceinline__ void for_row_copy(const unsigned short* __restrict__ row, int vocab,
                                             unsigned short* __restrict__ copy_to, F&& f) {
    int start = 0;
    if (((((uintptr_t)row) | (uintptr_t)copy_to) & 15) == 0) {
        const int nvec = vocab >> 3;
        for (int i = threadIdx.x; i < nvec; i += NT) {
            const u32x4 raw = reinterpret_cast<const u32x4*>(row)[i];
            if (copy_to) reinterpret_cast<u32x4*>(copy_to)[i] = raw;
#pragma unroll
            for (int e = 0; e < 8; ++e) f(i * 8 + e, (raw[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
        }
        start = nvec << 3;
    }
    for (int v = start + threadIdx.x; v < vocab; v += NT) {
        const unsigned short b = row[v];
        if (copy_to) copy_to[v] = b;
        f(v, (uint32_t)b);
    }
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

// ---- per-request parameters (header, K11 "per request"): T, top_p and top_k are read from device memory
constexpr uint32_t kGreedyMark = 0x10000u;  // kstar of a greedy row's stored stats: above every 16-bit key

struct SmemReq {
    Smem s;
    unsigned long long lo[256];  // masses by the low byte inside the top-k bin
    uint32_t cnt[256];           // token counts beside the mass histogram of the same pass
};

// out-of-range device values never fault: top_p outside (0, 1) (NaN included) is 1, top_k outside [1, vocab) is off (0)
__device__ __forceinline__ float clean_top_p(float top_p) { return (top_p > 0.f && top_p < 1.f) ? top_p : 1.f; }
__device__ __forceinline__ int clean_top_k(const int32_t* top_k, int b, int vocab) {
    if (!top_k) return 0;
    const int k = top_k[b];
    return (k >= 1 && k < vocab) ? k : 0;
}

// wave 0: sel = min i such that base + sum_{j > i} cnt[j] < want (exists: i = 255 qualifies whenever base < want),
// above = that count.  scan_select on counts; the k-th largest key lies in bin sel when the bins hold >= want - base.
__device__ void count_select(const uint32_t* cnt, uint32_t base, uint32_t want, Smem& s) {
    if (threadIdx.x < 64) {
        const int l = threadIdx.x;
        uint32_t h[4], own = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            h[e] = cnt[4 * l + e];
            own += h[e];
        }
        uint32_t incl = own;  // sum over lanes >= l
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_down(incl, o);
            if (l + o < 64) incl += t;
        }
        uint32_t acc = base + (incl - own);
        int n = 0, sel_here = -1;
        uint32_t above_here = 0;
#pragma unroll
        for (int e = 3; e >= 0; --e) {
            if (acc < want) {
                ++n;
                sel_here = 4 * l + e;
                above_here = acc;
            }
            acc += h[e];
        }
        int total = n;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o);
        const int sel = 256 - total;
        if (total == 0 && l == 0) {     // unreachable for base < want; keeps s.sel defined
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

// row_stats with a top-k count select first (1 <= k < vocab): the stats of the row whose tokens below the k-th largest
// key are -inf.  Passes: max; high-byte masses and counts; low byte inside the top-k bin (kstar_k, Z_k); then, when
// top_p < 1, the high-byte select with thr = top_p * Z_k and the low byte inside the top-p bin -- from the masses
// already in LDS when both bins coincide, else one more pass.  Result in q.s.st; its kstar is never below kstar_k.
template <int NT>
__device__ void row_stats_topk(const unsigned short* __restrict__ row, int vocab, float invT, float top_p, int k,
                               SmemReq& q) {
    Smem& s = q.s;
    float mx = -INFINITY;
    for_row<NT>(row, vocab, [&](int, uint32_t b) { mx = fmaxf(mx, bf16_bits_to_f32(b)); });
    mx = block_max<NT>(mx, s);
    for (int i = threadIdx.x; i < 256; i += NT) {
        s.hist[i] = 0;
        q.cnt[i] = 0;
    }
    __syncthreads();
    for_row<NT>(row, vocab, [&](int, uint32_t b) {
        const uint32_t hi = key16(b) >> 8;
        atomicAdd(&q.cnt[hi], 1u);
        const unsigned long long w = mass_fx(bf16_bits_to_f32(b), mx, invT);
        if (w) atomicAdd(&s.hist[hi], w);
    });
    __syncthreads();
    count_select(q.cnt, 0u, (uint32_t)k, s);
    const int hbk = s.sel;
    const uint32_t count_above = (uint32_t)s.above;
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += NT) {
        q.lo[i] = 0;
        q.cnt[i] = 0;
    }
    __syncthreads();
    for_row<NT>(row, vocab, [&](int, uint32_t b) {
        const uint32_t key = key16(b);
        if ((int)(key >> 8) == hbk) {
            atomicAdd(&q.cnt[key & 0xffu], 1u);
            const unsigned long long w = mass_fx(bf16_bits_to_f32(b), mx, invT);
            if (w) atomicAdd(&q.lo[key & 0xffu], w);
        }
    });
    __syncthreads();
    count_select(q.cnt, count_above, (uint32_t)k, s);
    const int lbk = s.sel;
    __syncthreads();
    // the high-byte histogram of the masked row: nothing below bin hbk, the survivors' mass in it; Z_k by a tree
    for (int i = threadIdx.x; i < 256; i += NT) {
        if (i < hbk) s.hist[i] = 0;
        if (i < lbk) q.lo[i] = 0;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        unsigned long long in_bin = 0, z = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = 4 * threadIdx.x + e;
            in_bin += q.lo[i];
            if (i != hbk) z += s.hist[i];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            in_bin += __shfl_xor(in_bin, o);
            z += __shfl_xor(z, o);
        }
        if (threadIdx.x == 0) {
            s.hist[hbk] = in_bin;
            s.above = z + in_bin;
            if (top_p >= 1.f) s.st = RowStats{mx, ((uint32_t)hbk << 8) | (uint32_t)lbk, z + in_bin};
        }
    }
    __syncthreads();
    if (top_p >= 1.f) return;
    const unsigned long long Z = s.above;
    const double thr = (double)top_p * (double)Z;
    __syncthreads();
    scan_select(s, 0ull, thr);
    const int hb = s.sel;   // >= hbk: the bins below hold nothing and Z_k > thr
    const unsigned long long above_hb = s.above;
    __syncthreads();
    if (hb == hbk) {
        for (int i = threadIdx.x; i < 256; i += NT) s.hist[i] = q.lo[i];
    } else {
        for (int i = threadIdx.x; i < 256; i += NT) s.hist[i] = 0;
        __syncthreads();
        for_row<NT>(row, vocab, [&](int, uint32_t b) {
            const uint32_t key = key16(b);
            if ((int)(key >> 8) == hb) {
                const unsigned long long w = mass_fx(bf16_bits_to_f32(b), mx, invT);
                if (w) atomicAdd(&s.hist[key & 0xffu], w);
            }
        });
    }
    __syncthreads();
    scan_select(s, above_hb, thr);
    if (threadIdx.x == 0) s.st = RowStats{mx, ((uint32_t)hb << 8) | (uint32_t)s.sel, s.above + s.hist[s.sel]};
    __syncthreads();
}

// the filter of request parameters (T > 0): row_stats itself when top-k is off.  Inlined into its kernels: as a
// function of its own it calls row_stats and has to spill its return address, which gives the kernels a scratch segment
template <int NT>
__device__ __forceinline__ void row_stats_req(const unsigned short* __restrict__ row, int vocab, float invT,
                                              float top_p, int k, SmemReq& q) {
    if (k)
        row_stats_topk<NT>(row, vocab, invT, top_p, k, q);
    else
        row_stats<NT>(row, vocab, invT, top_p, q.s);
}

// a greedy row: md_argmax's token (largest value, lowest index among equal ones, 0 if nothing compares above -inf);
// optionally copies the row to `copy_to`
template <int NT>
__device__ int argmax_row(const unsigned short* __restrict__ row, int vocab, Smem& s,
                          unsigned short* __restrict__ copy_to) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    auto visit = [&](int v, uint32_t b) {
        const float x = bf16_bits_to_f32(b);
        if (x > best || (x == best && v < bi)) {
            best = x;
            bi = v;
        }
    };
    for_row_copy<NT>(row, vocab, copy_to, visit);
    const int t = block_argmax<NT>(best, bi, s);
    return t < 0 ? 0 : t;
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
    for_row_copy<NT>(row, vocab, copy_to, visit);
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

struct RequestParams {      // [B] each, device memory, read at launch time
    const float* T;
    const float* top_p;
    const int32_t* top_k;   // or null: off
};

// sample_rows_kernel with request b's own (T, top_p, top_k).  A request whose T is not > 0 is greedy: its token is the
// row's argmax; in draft mode its row still goes to the ring, with stats {m, kGreedyMark, 0} that no verify reads.
template <int NT>
__global__ __launch_bounds__(NT) void sample_rows_req_kernel(const SampleParams p, const RequestParams rp) {
    __shared__ SmemReq q;
    Smem& s = q.s;
    const int b = blockIdx.x;
    read_counters(p.counters, s);
    int r = p.n - 1;
    if (p.row_sel) {
        const int64_t sel = p.row_sel[b] - 1;
        r = sel < 0 ? 0 : (sel >= p.n ? p.n - 1 : (int)sel);
    }
    const unsigned short* row = p.logits + ((int64_t)b * p.n + r) * p.row_stride;
    const bool draft = p.ring != nullptr;
    const int j = draft ? (int)s.step : 0;
    const bool store = draft && j >= 0 && j < p.gamma;
    unsigned short* copy_to = store ? p.ring + ((int64_t)b * p.gamma + j) * p.vocab : nullptr;
    const float T = rp.T[b];
    RowStats st;
    int tok;
    if (T > 0.f) {      // uniform over the workgroup: one request each
        const float invT = 1.0f / T;
        row_stats_req<NT>(row, p.vocab, invT, clean_top_p(rp.top_p[b]), clean_top_k(rp.top_k, b, p.vocab), q);
        st = s.st;
        const NoiseKey nk = noise_key(p.seed, p.purpose, j, b, s.iter);
        tok = draw_row<NT>(row, p.vocab, st, invT, nk, s, copy_to);
    } else {
        tok = argmax_row<NT>(row, p.vocab, s, copy_to);
        st = RowStats{bf16_bits_to_f32(row[tok]), kGreedyMark, 0ull};
    }
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

// row_stats_kernel with the parameters of the row's request b = row / (gamma + 1).  A greedy request's rows get
// {m, kGreedyMark, argmax of the row} instead: spec_verify_req_kernel copies the token out.
template <int NT>
__global__ __launch_bounds__(NT) void row_stats_req_kernel(const unsigned short* __restrict__ logits,
                                                           int64_t row_stride, int vocab, int gamma,
                                                           const RequestParams rp, RowStats* out) {
    __shared__ SmemReq q;
    const int b = blockIdx.x / (gamma + 1);
    const unsigned short* row = logits + (int64_t)blockIdx.x * row_stride;
    const float T = rp.T[b];
    if (T > 0.f) {
        row_stats_req<NT>(row, vocab, 1.0f / T, clean_top_p(rp.top_p[b]), clean_top_k(rp.top_k, b, vocab), q);
        if (threadIdx.x == 0) out[blockIdx.x] = q.s.st;
    } else {
        const int tok = argmax_row<NT>(row, vocab, q.s, nullptr);
        if (threadIdx.x == 0)
            out[blockIdx.x] = RowStats{bf16_bits_to_f32(row[tok]), kGreedyMark, (unsigned long long)tok};
    }
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
__device__ __forceinline__ void verify_request(const VerifyParams& p, const float invT, Smem& s) {
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
            const float pd = prob_of(trow(j)[d], p.target_stats[(int64_t)b * (G + 1) + j], invT);
            const float qd = prob_of(rrow(j)[d], p.ring_stats[(int64_t)b * G + j], invT);
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
            const float r = prob_of(tr[v], ps, invT) - prob_of(rr[v], qs, invT);
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
                const float sc = (bf16_bits_to_f32(bits) - ps.m) * invT + gumbel_of(pick(w, v));
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
        tok = draw_row<NT>(trow(G), p.vocab, p.target_stats[(int64_t)b * (G + 1) + G], invT, nk, s, nullptr);
    }
    if (threadIdx.x == 0) {
        int64_t* tt = p.target_tokens + (int64_t)b * (G + 1);
        for (int j = 0; j <= G; ++j) tt[j] = j < jr ? tb[j + 1] : (j == jr ? (int64_t)tok : (int64_t)-1);
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void spec_verify_kernel(const VerifyParams p) {
    __shared__ Smem s;
    verify_request<NT>(p, p.invT, s);
    ticket_advance(p.counters, MD_SAMPLE_ADVANCE_ITER);
}

// spec_verify_kernel with request b's own T (its filter is in the stats row_stats_req_kernel wrote).  A greedy request
// gets target_tokens[b, j] = argmax of target row j for every j, what the greedy loop hands the accept kernel; its ring
// slots are not read.
template <int NT>
__global__ __launch_bounds__(NT) void spec_verify_req_kernel(const VerifyParams p, const float* __restrict__ T) {
    __shared__ Smem s;
    const int b = blockIdx.x, G = p.gamma;
    const float t = T[b];
    if (t > 0.f) {      // uniform over the workgroup
        verify_request<NT>(p, 1.0f / t, s);
    } else if (threadIdx.x == 0) {
        for (int j = 0; j <= G; ++j)
            p.target_tokens[(int64_t)b * (G + 1) + j] = (int64_t)p.target_stats[(int64_t)b * (G + 1) + j].zkept;
    }
    ticket_advance(p.counters, MD_SAMPLE_ADVANCE_ITER);
}

bool wide(int rows, int vocab) { return rows <= 512 && vocab >= 16384; }

// ------------------------------------------------------------------------------------------------------------------
// Vocab-sharded form (tensor parallelism): a rank holds the columns [vocab_offset, vocab_offset + v_loc) of every row.
// A logical call is a chain of launches with ONE all-reduce of a small int64 device tensor between two of them
// (header, K11 "sharded"): max (+ verify probe) -> MAX, high-byte histogram -> SUM, low-byte histogram -> SUM
// (top_p < 1 only), local candidates -> MAX, finish.  Every quantity that crosses ranks is an integer or an order key,
// so the reduced values -- hence the stats, jr and the tokens -- are the bits of the one-GPU kernels on the whole row.

// the inverse of key16
__device__ __forceinline__ uint32_t bits_of_key16(uint32_t k) { return (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu); }

constexpr long long kNoCand = -1;
// (score, global index) as an int64 whose signed order is (score ascending, index descending); -0 counts as +0, as in
// the float compare of block_argmax.  63 bits: never negative, so kNoCand is below every candidate.
__device__ __forceinline__ long long pack_cand(float sc, int v) {
    if (v < 0) return kNoCand;
    uint32_t u = __float_as_uint(sc);
    if ((u << 1) == 0) u = 0;
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return (long long)(((unsigned long long)u << 31) | (unsigned long long)(0x7fffffff - v));
}
__device__ __forceinline__ int cand_index(long long c) { return 0x7fffffff - (int)(c & 0x7fffffffll); }

// block_argmax that also returns the winning score: (best, bi) of the block in every thread, bi = -1 if best is -inf
template <int NT>
__device__ void block_argmax_sc(float& best, int& bi, Smem& s) {
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
    if (best == -INFINITY) bi = -1;
}

// the drawn row of request b: row_sel[b] - 1 of its n rows, else the last
__device__ __forceinline__ const unsigned short* shard_row(const unsigned short* logits, int64_t row_stride, int n,
                                                           const int64_t* row_sel, int b) {
    int r = n - 1;
    if (row_sel) {
        const int64_t q = row_sel[b] - 1;
        r = q < 0 ? 0 : (q >= n ? n - 1 : (int)q);
    }
    return logits + ((int64_t)b * n + r) * row_stride;
}

// Stats of a row from its reduced quantities, as row_stats derives them from the row itself: Z from the high-byte
// histogram, hb / above_hb by scan_select, then (unless only_hb) kstar and Z_kept from the low-byte histogram of bin hb.
// Result in s.st (only_hb: s.sel = hb, s.above = above_hb; returns thr).
__device__ double derive_stats(float mx, const long long* __restrict__ hi, const long long* __restrict__ lo,
                               float top_p, bool only_hb, Smem& s) {
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s.hist[i] = (unsigned long long)hi[i];
    __syncthreads();
    if (threadIdx.x < 64) {
        unsigned long long z = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) z += s.hist[4 * threadIdx.x + e];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o);
        if (threadIdx.x == 0) {
            s.above = z;
            if (top_p >= 1.f) s.st = RowStats{mx, 0u, z};
        }
    }
    __syncthreads();
    if (top_p >= 1.f) return 0.0;
    const unsigned long long Z = s.above;
    const double thr = (double)top_p * (double)Z;
    __syncthreads();
    scan_select(s, 0ull, thr);
    if (only_hb) return thr;
    const int hb = s.sel;
    const unsigned long long above_hb = s.above;
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s.hist[i] = (unsigned long long)lo[i];
    __syncthreads();
    scan_select(s, above_hb, thr);
    if (threadIdx.x == 0) s.st = RowStats{mx, ((uint32_t)hb << 8) | (uint32_t)s.sel, s.above + s.hist[s.sel]};
    __syncthreads();
    return thr;
}

struct ShardParams {
    const unsigned short* logits;   // this rank's columns of [R*n, row_stride]
    int64_t row_stride;
    int R, n, v_loc, vocab_offset, vocab_total, gamma, purpose;
    float invT, top_p;
    uint64_t seed;
    const int64_t* row_sel;
    const int64_t* tokens_buffer;   // [B, gamma+1] (verify)
    const unsigned short* ring;     // verify: row (b, j) at ring + (b*gamma + j) * ring_row_stride + ring_col_offset
    int64_t ring_row_stride, ring_col_offset;
    unsigned short* ring_out;       // draft: this rank's ring shard [B, gamma, v_loc]
    RowStats* ring_stats;           // [B, gamma]
    RowStats* target_stats;         // [B*(gamma+1)]
    int32_t* counters;
    const long long* red_max;       // reduced phase-A tensor
    const long long* hist_hi;       // reduced [R, 256]
    const long long* hist_lo;       // reduced [R, 256] (top_p < 1)
    long long* out;                 // this phase's tensor to reduce
};

// phase A: key of the shard's max per row; verify: the probe of the draft token d of (b, j), written by its owner
template <int NT>
__global__ __launch_bounds__(NT) void shard_max_kernel(const ShardParams p) {
    __shared__ Smem s;
    const int row = blockIdx.x;
    const unsigned short* lr = shard_row(p.logits, p.row_stride, p.n, p.row_sel, row);
    float mx = -INFINITY;
    for_row<NT>(lr, p.v_loc, [&](int, uint32_t b) { mx = fmaxf(mx, bf16_bits_to_f32(b)); });
    mx = block_max<NT>(mx, s);
    if (threadIdx.x == 0) {
        p.out[row] = (long long)key16(__float_as_uint(mx) >> 16);
        if (p.tokens_buffer) {
            const int G = p.gamma, b = row / (G + 1), j = row % (G + 1);
            if (j < G) {
                const int64_t d = p.tokens_buffer[(int64_t)b * (G + 1) + j + 1];
                long long probe = 0;
                if (d >= 0 && d < p.vocab_total && d >= p.vocab_offset && d < (int64_t)p.vocab_offset + p.v_loc) {
                    const int64_t c = d - p.vocab_offset;
                    const unsigned short* rr = p.ring + ((int64_t)b * G + j) * p.ring_row_stride + p.ring_col_offset;
                    probe = (1ll << 32) | ((long long)lr[c] << 16) | (long long)rr[c];
                }
                p.out[(int64_t)p.R + (int64_t)b * G + j] = probe;
            }
        }
    }
}

// phase B (hist_hi == null): masses by the high byte of the key, under the global max; phase C: by the low byte inside
// the bin hb that every rank derives from the reduced phase-B row
template <int NT>
__global__ __launch_bounds__(NT) void shard_hist_kernel(const ShardParams p) {
    __shared__ Smem s;
    const int row = blockIdx.x;
    const unsigned short* lr = shard_row(p.logits, p.row_stride, p.n, p.row_sel, row);
    const float mx = bf16_bits_to_f32((unsigned short)bits_of_key16((uint32_t)p.red_max[row]));
    int hb = -1;
    if (p.hist_hi) {
        derive_stats(mx, p.hist_hi + (int64_t)row * 256, nullptr, p.top_p, true, s);
        hb = s.sel;
        __syncthreads();
    }
    for (int i = threadIdx.x; i < 256; i += NT) s.hist[i] = 0;
    __syncthreads();
    if (hb < 0) {
        for_row<NT>(lr, p.v_loc, [&](int, uint32_t b) {
            const unsigned long long w = mass_fx(bf16_bits_to_f32(b), mx, p.invT);
            if (w) atomicAdd(&s.hist[key16(b) >> 8], w);
        });
    } else {
        for_row<NT>(lr, p.v_loc, [&](int, uint32_t b) {
            const uint32_t k = key16(b);
            if ((int)(k >> 8) == hb) {
                const unsigned long long w = mass_fx(bf16_bits_to_f32(b), mx, p.invT);
                if (w) atomicAdd(&s.hist[k & 0xffu], w);
            }
        });
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += NT) p.out[(int64_t)row * 256 + i] = (long long)s.hist[i];
}

// Gumbel-max over this shard's kept tokens, noise and index by the global v = voff + local; -> (best, bi) in every thread
template <int NT>
__device__ void draw_shard(const unsigned short* __restrict__ row, int v_loc, int voff, const RowStats& st, float invT,
                           const NoiseKey& nk, Smem& s, unsigned short* __restrict__ copy_to, float& best, int& bi) {
    best = -INFINITY;
    bi = 0x7fffffff;
    int grp = -1;
    Word4 w{0, 0, 0, 0};
    auto visit = [&](int vl, uint32_t b) {
        if (key16(b) < st.kstar) return;
        const int v = voff + vl;
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
        const int nvec = v_loc >> 3;
        for (int i = threadIdx.x; i < nvec; i += NT) {
            const u32x4 raw = reinterpret_cast<const u32x4*>(row)[i];
            if (copy_to) reinterpret_cast<u32x4*>(copy_to)[i] = raw;
#pragma unroll
            for (int e = 0; e < 8; ++e) visit(i * 8 + e, (raw[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
        }
        start = nvec << 3;
    }
    for (int vl = start + threadIdx.x; vl < v_loc; vl += NT) {
        const unsigned short b = row[vl];
        if (copy_to) copy_to[vl] = b;
        visit(vl, (uint32_t)b);
    }
    block_argmax_sc<NT>(best, bi, s);
}

// phase D of a draw: stats from the reduced histograms (identical on every rank), the local candidate, the ring shard
template <int NT>
__global__ __launch_bounds__(NT) void shard_draw_kernel(const ShardParams p) {
    __shared__ Smem s;
    const int b = blockIdx.x;
    read_counters(p.counters, s);
    const unsigned short* lr = shard_row(p.logits, p.row_stride, p.n, p.row_sel, b);
    const float mx = bf16_bits_to_f32((unsigned short)bits_of_key16((uint32_t)p.red_max[b]));
    derive_stats(mx, p.hist_hi + (int64_t)b * 256, p.hist_lo ? p.hist_lo + (int64_t)b * 256 : nullptr, p.top_p, false, s);
    const RowStats st = s.st;
    const bool draft = p.ring_out != nullptr;
    const int j = draft ? (int)s.step : 0;
    const bool store = draft && j >= 0 && j < p.gamma;
    unsigned short* copy_to = store ? p.ring_out + ((int64_t)b * p.gamma + j) * p.v_loc : nullptr;
    const NoiseKey nk = noise_key(p.seed, p.purpose, j, b, s.iter);
    float best;
    int bi;
    draw_shard<NT>(lr, p.v_loc, p.vocab_offset, st, p.invT, nk, s, copy_to, best, bi);
    if (threadIdx.x == 0) {
        p.out[b] = pack_cand(best, bi);
        if (store) p.ring_stats[(int64_t)b * p.gamma + j] = st;
    }
}

// phase E of a draw: the global winner (token 0 if nothing was kept anywhere) to all n columns; advances the counters
__global__ __launch_bounds__(256) void shard_draw_finish_kernel(const long long* __restrict__ cand, int B, int n,
                                                                int32_t* counters, int advance, int64_t* out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) {
        const long long c = cand[b];
        const int64_t tok = c < 0 ? 0 : (int64_t)cand_index(c);
        for (int k = 0; k < n; ++k) out[(int64_t)b * n + k] = tok;
    }
    ticket_advance(counters, advance);
}

// phase D of a verify: target stats of the request's gamma + 1 rows, the accept walk from the probes (the same jr on
// every rank), then this shard's candidates: [b, 0] the residual draw at jr or the bonus draw, [b, 1] the fallback
// (p~ without d) at jr, [b, 2] = jr.
template <int NT>
__global__ __launch_bounds__(NT) void shard_verify_kernel(const ShardParams p) {
    __shared__ Smem s;
    const int b = blockIdx.x, G = p.gamma;
    read_counters(p.counters, s);
    const uint32_t iter = s.iter;
    const int64_t* tb = p.tokens_buffer + (int64_t)b * (G + 1);
    for (int j = 0; j <= G; ++j) {
        const int64_t row = (int64_t)b * (G + 1) + j;
        const float mx = bf16_bits_to_f32((unsigned short)bits_of_key16((uint32_t)p.red_max[row]));
        derive_stats(mx, p.hist_hi + row * 256, p.hist_lo ? p.hist_lo + row * 256 : nullptr, p.top_p, false, s);
        if (threadIdx.x == 0) p.target_stats[row] = s.st;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int jr = G;
        for (int j = 0; j < G; ++j) {
            const long long probe = p.red_max[(int64_t)p.R + (int64_t)b * G + j];
            if (!((probe >> 32) & 1)) {     // d owned by no rank: outside [0, vocab_total)
                jr = j;
                break;
            }
            const float pd = prob_of((uint32_t)(probe >> 16) & 0xffffu, p.target_stats[(int64_t)b * (G + 1) + j], p.invT);
            const float qd = prob_of((uint32_t)probe & 0xffffu, p.ring_stats[(int64_t)b * G + j], p.invT);
            const NoiseKey nk = noise_key(p.seed, MD_SAMPLE_ACCEPT, j, b, iter);
            const float u = uniform_of(noise_block(nk, 0).x);
            if (!(u * qd < pd)) {
                jr = j;
                break;
            }
        }
        s.jr = jr;
        s.st = p.target_stats[(int64_t)b * (G + 1) + jr];
    }
    __syncthreads();
    const int jr = s.jr;
    const RowStats ps = s.st;
    const unsigned short* tr = p.logits + ((int64_t)b * (G + 1) + jr) * p.row_stride;
    float best, fbest = -INFINITY;
    int bi, fbi = -1;
    if (jr < G) {
        const RowStats qs = p.ring_stats[(int64_t)b * G + jr];
        const int64_t d = tb[jr + 1];
        const unsigned short* rr = p.ring + ((int64_t)b * G + jr) * p.ring_row_stride + p.ring_col_offset;
        const NoiseKey nk = noise_key(p.seed, MD_SAMPLE_RESIDUAL, jr, b, iter);
        best = -INFINITY;
        bi = 0x7fffffff;
        fbi = 0x7fffffff;
        int grp = -1;
        Word4 w{0, 0, 0, 0};
        for (int vl = threadIdx.x; vl < p.v_loc; vl += NT) {
            const uint32_t bits = tr[vl];
            const int v = p.vocab_offset + vl;
            const float r = prob_of(bits, ps, p.invT) - prob_of(rr[vl], qs, p.invT);
            const bool res = r > 0.f;
            const bool fb = !(v == d || key16(bits) < ps.kstar);
            if (!res && !fb) continue;
            if ((v >> 2) != grp) {
                grp = v >> 2;
                w = noise_block(nk, v);
            }
            const float g = gumbel_of(pick(w, v));
            if (res) {
                const float sc = logf(r) + g;
                if (sc > best || (sc == best && v < bi)) {
                    best = sc;
                    bi = v;
                }
            }
            if (fb) {
                const float sc = (bf16_bits_to_f32(bits) - ps.m) * p.invT + g;
                if (sc > fbest || (sc == fbest && v < fbi)) {
                    fbest = sc;
                    fbi = v;
                }
            }
        }
        block_argmax_sc<NT>(best, bi, s);
        block_argmax_sc<NT>(fbest, fbi, s);
    } else {
        const NoiseKey nk = noise_key(p.seed, MD_SAMPLE_BONUS, G, b, iter);
        draw_shard<NT>(tr, p.v_loc, p.vocab_offset, ps, p.invT, nk, s, nullptr, best, bi);
    }
    if (threadIdx.x == 0) {
        p.out[(int64_t)b * 3] = pack_cand(best, bi);
        p.out[(int64_t)b * 3 + 1] = pack_cand(fbest, fbi);
        p.out[(int64_t)b * 3 + 2] = jr;
    }
}

// phase E of a verify: the last-resort rules of spec_verify_kernel on the global candidates, target_tokens in its encoding
__global__ __launch_bounds__(256) void shard_verify_finish_kernel(const long long* __restrict__ cand,
                                                                  const int64_t* __restrict__ tokens_buffer, int B, int G,
                                                                  int32_t* counters, int64_t* target_tokens) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) {
        const int64_t* tb = tokens_buffer + (int64_t)b * (G + 1);
        const long long c0 = cand[(int64_t)b * 3], c1 = cand[(int64_t)b * 3 + 1];
        long long jr = cand[(int64_t)b * 3 + 2];
        jr = jr < 0 ? 0 : (jr > G ? G : jr);
        int64_t tok;
        if (c0 >= 0)
            tok = cand_index(c0);
        else if (jr == G)
            tok = 0;
        else if (c1 >= 0)
            tok = cand_index(c1);
        else
            tok = tb[jr + 1] == 0 ? 1 : 0;
        int64_t* tt = target_tokens + (int64_t)b * (G + 1);
        for (int j = 0; j <= G; ++j) tt[j] = j < jr ? tb[j + 1] : (j == jr ? tok : (int64_t)-1);
    }
    ticket_advance(counters, MD_SAMPLE_ADVANCE_ITER);
}

// what every phase reads: this rank's columns of the rows, and which row of a request is drawn
ShardParams shard_params(const void* logits, int64_t row_stride, int R, int n, int v_loc, const int64_t* row_sel) {
    ShardParams p{};
    p.logits = (const unsigned short*)logits;
    p.row_stride = row_stride;
    p.R = R;
    p.n = n;
    p.v_loc = v_loc;
    p.row_sel = row_sel;
    return p;
}

void shard_columns(ShardParams& p, int vocab_offset, int vocab_total) {
    p.vocab_offset = vocab_offset;
    p.vocab_total = vocab_total;
}

void shard_filter(ShardParams& p, float temperature, float top_p) {
    p.invT = 1.0f / temperature;
    p.top_p = top_p;
}

void shard_reduced(ShardParams& p, const int64_t* red_max, const int64_t* hist_hi, const int64_t* hist_lo) {
    p.red_max = (const long long*)red_max;
    p.hist_hi = (const long long*)hist_hi;
    p.hist_lo = (const long long*)hist_lo;
}

// the verify's view of the draft ring: a ring shard, or this rank's columns of a full ring
void shard_ring_view(ShardParams& p, const int64_t* tokens_buffer, const void* ring, int64_t ring_row_stride,
                     int64_t ring_col_offset) {
    p.tokens_buffer = tokens_buffer;
    p.ring = (const unsigned short*)ring;
    p.ring_row_stride = ring_row_stride;
    p.ring_col_offset = ring_col_offset;
}

#define MD_SHARD_LAUNCH(kernel, rows, grid, p, stream, what)                                                 \
    do {                                                                                                     \
        if (wide(rows, (p).v_loc))                                                                           \
            hipLaunchKernelGGL((kernel<1024>), dim3(grid), dim3(1024), 0, (hipStream_t)(stream), p);         \
        else                                                                                                 \
            hipLaunchKernelGGL((kernel<256>), dim3(grid), dim3(256), 0, (hipStream_t)(stream), p);           \
        MD_CHECK_LAUNCH(what);                                                                               \
    } while (0)

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

// ---- per-request entry points (header, K11 "per request"): T / top_p / top_k are device tensors of B values, so no
// value is checked here; the kernels map every out-of-range value to a defined setting
extern "C" int md_sample_rows_req(const void* logits, int64_t row_stride, int B, int n, int vocab,
                                  const float* temperature, const float* top_p, const int32_t* top_k, uint64_t seed,
                                  int purpose, const int64_t* row_sel, int32_t* counters, int advance, void* ring,
                                  void* ring_stats, int gamma, int64_t* tokens_out, md_stream_t stream) {
    MD_CHECK_ARG(logits && temperature && top_p && counters && tokens_out, "md_sample_rows_req: null pointer argument");
    MD_CHECK_ARG(B > 0 && n > 0 && vocab > 0 && row_stride >= 0, "md_sample_rows_req: bad shape B=%d n=%d vocab=%d", B,
                 n, vocab);
    MD_CHECK_ARG(purpose >= 0 && purpose <= MD_SAMPLE_BONUS, "md_sample_rows_req: bad purpose %d", purpose);
    MD_CHECK_ARG(advance >= MD_SAMPLE_ADVANCE_NONE && advance <= MD_SAMPLE_ADVANCE_ITER,
                 "md_sample_rows_req: bad advance mode %d", advance);
    MD_CHECK_ARG((ring == nullptr) == (ring_stats == nullptr), "md_sample_rows_req: ring and ring_stats go together");
    MD_CHECK_ARG(ring == nullptr || gamma >= 1, "md_sample_rows_req: a draft ring needs gamma >= 1");
    SampleParams p;
    p.logits = (const unsigned short*)logits;
    p.row_stride = row_stride;
    p.n = n;
    p.vocab = vocab;
    p.purpose = purpose;
    p.advance = advance;
    p.gamma = gamma;
    p.invT = 0.f;   // unused: the kernel reads the request's own
    p.top_p = 0.f;
    p.seed = seed;
    p.row_sel = row_sel;
    p.counters = counters;
    p.ring = (unsigned short*)ring;
    p.ring_stats = (RowStats*)ring_stats;
    p.out = tokens_out;
    const RequestParams rp{temperature, top_p, top_k};
    if (wide(B, vocab))
        hipLaunchKernelGGL((sample_rows_req_kernel<1024>), dim3(B), dim3(1024), 0, (hipStream_t)stream, p, rp);
    else
        hipLaunchKernelGGL((sample_rows_req_kernel<256>), dim3(B), dim3(256), 0, (hipStream_t)stream, p, rp);
    MD_CHECK_LAUNCH("md_sample_rows_req");
    return MD_OK;
}

extern "C" int md_spec_verify_sample_req(const void* logits, int64_t row_stride, int B, int gamma, int vocab,
                                         const float* temperature, const float* top_p, const int32_t* top_k,
                                         uint64_t seed, const int64_t* tokens_buffer, const void* ring,
                                         const void* ring_stats, void* target_stats, int32_t* counters,
                                         int64_t* target_tokens, md_stream_t stream) {
    MD_CHECK_ARG(logits && temperature && top_p && tokens_buffer && ring && ring_stats && target_stats && counters &&
                     target_tokens,
                 "md_spec_verify_sample_req: null pointer argument");
    MD_CHECK_ARG(B > 0 && gamma >= 1 && vocab > 0 && row_stride >= vocab && (int64_t)B * (gamma + 1) <= 0x7fffffff,
                 "md_spec_verify_sample_req: bad shape B=%d gamma=%d vocab=%d", B, gamma, vocab);
    const int rows = B * (gamma + 1);
    const RequestParams rp{temperature, top_p, top_k};
    if (wide(rows, vocab))
        hipLaunchKernelGGL((row_stats_req_kernel<1024>), dim3(rows), dim3(1024), 0, (hipStream_t)stream,
                           (const unsigned short*)logits, row_stride, vocab, gamma, rp, (RowStats*)target_stats);
    else
        hipLaunchKernelGGL((row_stats_req_kernel<256>), dim3(rows), dim3(256), 0, (hipStream_t)stream,
                           (const unsigned short*)logits, row_stride, vocab, gamma, rp, (RowStats*)target_stats);
    MD_CHECK_LAUNCH("md_spec_verify_sample_req(stats)");
    VerifyParams p;
    p.logits = (const unsigned short*)logits;
    p.row_stride = row_stride;
    p.gamma = gamma;
    p.vocab = vocab;
    p.invT = 0.f;   // unused: the kernel reads the request's own
    p.seed = seed;
    p.tokens_buffer = tokens_buffer;
    p.ring = (const unsigned short*)ring;
    p.ring_stats = (const RowStats*)ring_stats;
    p.target_stats = (const RowStats*)target_stats;
    p.counters = counters;
    p.target_tokens = target_tokens;
    if (wide(B, vocab))
        hipLaunchKernelGGL((spec_verify_req_kernel<1024>), dim3(B), dim3(1024), 0, (hipStream_t)stream, p, temperature);
    else
        hipLaunchKernelGGL((spec_verify_req_kernel<256>), dim3(B), dim3(256), 0, (hipStream_t)stream, p, temperature);
    MD_CHECK_LAUNCH("md_spec_verify_sample_req");
    return MD_OK;
}

// ---- vocab-sharded entry points (header, K11 "sharded"): the local phases; the caller all-reduces between them
#define MD_SHARD_CHECK_SHAPE(name)                                                                                   \
    MD_CHECK_ARG(R > 0 && n > 0 && v_loc > 0 && row_stride >= 0, name ": bad shape rows=%d n=%d v_loc=%d", R, n, v_loc)
#define MD_SHARD_CHECK_OFFSET(name)                                                                                  \
    MD_CHECK_ARG(vocab_offset >= 0 && vocab_total > 0 && (int64_t)vocab_offset + v_loc <= (int64_t)vocab_total,      \
                 name ": columns [%d, %d + %d) are not inside the vocabulary of %d", vocab_offset, vocab_offset,      \
                 v_loc, vocab_total)
#define MD_SHARD_CHECK_TP(name)                                                                                      \
    MD_CHECK_ARG(temperature > 0.f && top_p > 0.f && top_p <= 1.f,                                                   \
                 name ": need temperature > 0 and 0 < top_p <= 1 (got %g, %g)", temperature, top_p)

extern "C" int md_sample_shard_max(const void* logits, int64_t row_stride, int R, int n, int v_loc,
                                   const int64_t* row_sel, const int64_t* tokens_buffer, const void* ring,
                                   int64_t ring_row_stride, int64_t ring_col_offset, int gamma, int vocab_offset,
                                   int vocab_total, int64_t* red_out, md_stream_t stream) {
    MD_CHECK_ARG(logits && red_out, "md_sample_shard_max: null pointer argument");
    MD_SHARD_CHECK_SHAPE("md_sample_shard_max");
    MD_SHARD_CHECK_OFFSET("md_sample_shard_max");
    if (tokens_buffer) {
        MD_CHECK_ARG(ring && gamma >= 1 && n == 1 && row_sel == nullptr && R % (gamma + 1) == 0,
                     "md_sample_shard_max: the verify probe needs a ring, gamma >= 1 and rows = B (gamma + 1), n = 1");
        MD_CHECK_ARG(ring_col_offset >= 0 && ring_row_stride >= ring_col_offset + v_loc && row_stride >= v_loc,
                     "md_sample_shard_max: ring columns [%lld, +%d) exceed its row stride %lld",
                     (long long)ring_col_offset, v_loc, (long long)ring_row_stride);
    }
    ShardParams p = shard_params(logits, row_stride, R, n, v_loc, row_sel);
    shard_columns(p, vocab_offset, vocab_total);
    shard_ring_view(p, tokens_buffer, ring, ring_row_stride, ring_col_offset);
    p.gamma = gamma;
    p.out = (long long*)red_out;
    MD_SHARD_LAUNCH(shard_max_kernel, R, R, p, stream, "md_sample_shard_max");
    return MD_OK;
}

extern "C" int md_sample_shard_hist(const void* logits, int64_t row_stride, int R, int n, int v_loc,
                                    const int64_t* row_sel, float temperature, float top_p, const int64_t* red_max,
                                    const int64_t* hist_hi, int64_t* hist_out, md_stream_t stream) {
    MD_CHECK_ARG(logits && red_max && hist_out, "md_sample_shard_hist: null pointer argument");
    MD_SHARD_CHECK_SHAPE("md_sample_shard_hist");
    MD_SHARD_CHECK_TP("md_sample_shard_hist");
    MD_CHECK_ARG(hist_hi == nullptr || top_p < 1.f, "md_sample_shard_hist: top_p = 1 has no low-byte phase");
    ShardParams p = shard_params(logits, row_stride, R, n, v_loc, row_sel);
    shard_filter(p, temperature, top_p);
    shard_reduced(p, red_max, hist_hi, nullptr);
    p.out = (long long*)hist_out;
    MD_SHARD_LAUNCH(shard_hist_kernel, R, R, p, stream, "md_sample_shard_hist");
    return MD_OK;
}

extern "C" int md_sample_shard_draw(const void* logits, int64_t row_stride, int B, int n, int v_loc, int vocab_offset,
                                    int vocab_total, float temperature, float top_p, uint64_t seed, int purpose,
                                    const int64_t* row_sel, const int32_t* counters, const int64_t* red_max,
                                    const int64_t* hist_hi, const int64_t* hist_lo, void* ring, void* ring_stats,
                                    int gamma, int64_t* cand_out, md_stream_t stream) {
    const int R = B;
    MD_CHECK_ARG(logits && counters && red_max && hist_hi && cand_out, "md_sample_shard_draw: null pointer argument");
    MD_SHARD_CHECK_SHAPE("md_sample_shard_draw");
    MD_SHARD_CHECK_OFFSET("md_sample_shard_draw");
    MD_SHARD_CHECK_TP("md_sample_shard_draw");
    MD_CHECK_ARG((hist_lo != nullptr) == (top_p < 1.f),
                 "md_sample_shard_draw: the low-byte histogram goes with top_p < 1, and only with it");
    MD_CHECK_ARG(purpose >= 0 && purpose <= MD_SAMPLE_BONUS, "md_sample_shard_draw: bad purpose %d", purpose);
    MD_CHECK_ARG((ring == nullptr) == (ring_stats == nullptr), "md_sample_shard_draw: ring and ring_stats go together");
    MD_CHECK_ARG(ring == nullptr || gamma >= 1, "md_sample_shard_draw: a draft ring needs gamma >= 1");
    ShardParams p = shard_params(logits, row_stride, R, n, v_loc, row_sel);
    shard_columns(p, vocab_offset, vocab_total);
    shard_filter(p, temperature, top_p);
    shard_reduced(p, red_max, hist_hi, hist_lo);
    p.gamma = gamma;
    p.purpose = purpose;
    p.seed = seed;
    p.ring_out = (unsigned short*)ring;
    p.ring_stats = (RowStats*)ring_stats;
    p.counters = const_cast<int32_t*>(counters);
    p.out = (long long*)cand_out;
    MD_SHARD_LAUNCH(shard_draw_kernel, B, B, p, stream, "md_sample_shard_draw");
    return MD_OK;
}

extern "C" int md_sample_shard_finish(const int64_t* cand, int B, int n, int32_t* counters, int advance,
                                      int64_t* tokens_out, md_stream_t stream) {
    MD_CHECK_ARG(cand && counters && tokens_out, "md_sample_shard_finish: null pointer argument");
    MD_CHECK_ARG(B > 0 && n > 0, "md_sample_shard_finish: bad shape B=%d n=%d", B, n);
    MD_CHECK_ARG(advance >= MD_SAMPLE_ADVANCE_NONE && advance <= MD_SAMPLE_ADVANCE_ITER,
                 "md_sample_shard_finish: bad advance mode %d", advance);
    hipLaunchKernelGGL(shard_draw_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)cand, B, n, counters, advance, tokens_out);
    MD_CHECK_LAUNCH("md_sample_shard_finish");
    return MD_OK;
}

extern "C" int md_spec_verify_shard(const void* logits, int64_t row_stride, int B, int gamma, int v_loc,
                                    int vocab_offset, int vocab_total, float temperature, float top_p, uint64_t seed,
                                    const int64_t* tokens_buffer, const void* ring, int64_t ring_row_stride,
                                    int64_t ring_col_offset, const void* ring_stats, const int64_t* red_max,
                                    const int64_t* hist_hi, const int64_t* hist_lo, void* target_stats,
                                    const int32_t* counters, int64_t* cand_out, md_stream_t stream) {
    const int n = 1;
    MD_CHECK_ARG(logits && tokens_buffer && ring && ring_stats && red_max && hist_hi && target_stats && counters &&
                     cand_out,
                 "md_spec_verify_shard: null pointer argument");
    MD_CHECK_ARG(B > 0 && gamma >= 1 && (int64_t)B * (gamma + 1) <= 0x7fffffff,
                 "md_spec_verify_shard: bad shape B=%d gamma=%d", B, gamma);
    const int R = B * (gamma + 1);
    MD_SHARD_CHECK_SHAPE("md_spec_verify_shard");
    MD_CHECK_ARG(row_stride >= v_loc, "md_spec_verify_shard: row stride %lld below the local width %d",
                 (long long)row_stride, v_loc);
    MD_SHARD_CHECK_OFFSET("md_spec_verify_shard");
    MD_SHARD_CHECK_TP("md_spec_verify_shard");
    MD_CHECK_ARG((hist_lo != nullptr) == (top_p < 1.f),
                 "md_spec_verify_shard: the low-byte histogram goes with top_p < 1, and only with it");
    MD_CHECK_ARG(ring_col_offset >= 0 && ring_row_stride >= ring_col_offset + v_loc,
                 "md_spec_verify_shard: ring columns [%lld, +%d) exceed its row stride %lld", (long long)ring_col_offset,
                 v_loc, (long long)ring_row_stride);
    ShardParams p = shard_params(logits, row_stride, R, n, v_loc, nullptr);
    shard_columns(p, vocab_offset, vocab_total);
    shard_filter(p, temperature, top_p);
    shard_reduced(p, red_max, hist_hi, hist_lo);
    shard_ring_view(p, tokens_buffer, ring, ring_row_stride, ring_col_offset);
    p.gamma = gamma;
    p.seed = seed;
    p.ring_stats = (RowStats*)const_cast<void*>(ring_stats);
    p.target_stats = (RowStats*)target_stats;
    p.counters = const_cast<int32_t*>(counters);
    p.out = (long long*)cand_out;
    MD_SHARD_LAUNCH(shard_verify_kernel, B, B, p, stream, "md_spec_verify_shard");
    return MD_OK;
}

extern "C" int md_spec_verify_shard_finish(const int64_t* cand, const int64_t* tokens_buffer, int B, int gamma,
                                           int32_t* counters, int64_t* target_tokens, md_stream_t stream) {
    MD_CHECK_ARG(cand && tokens_buffer && counters && target_tokens, "md_spec_verify_shard_finish: null pointer argument");
    MD_CHECK_ARG(B > 0 && gamma >= 1, "md_spec_verify_shard_finish: bad shape B=%d gamma=%d", B, gamma);
    hipLaunchKernelGGL(shard_verify_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)cand, tokens_buffer, B, gamma, counters, target_tokens);
    MD_CHECK_LAUNCH("md_spec_verify_shard_finish");
    return MD_OK;
}
