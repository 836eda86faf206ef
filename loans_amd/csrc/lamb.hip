// LAMB (You et al. 2019, "Large Batch Optimization for Deep Learning", algorithm 2 with the identity for phi) over the flat
// parameter arena: Adam's direction with decoupled weight decay, its length set per segment by the trust ratio |p| / |u|.
//
// THE RULE.  Step t (1-based), gs = grad_scale.  Segment s has flag byte f: bit 0 = no weight decay, bit 1 = no adaptation
// (lars_segments' table).
//     g^  = g * gs
//     m'  = m + (1 - beta1) (g^ - m)
//     v'  = v + (1 - beta2) (g^ g^ - v)
//     c1  = 1 / (1 - beta1^t)      c2 = 1 / (1 - beta2^t)
//     a   = (m' c1) / (sqrt(v' c2) + eps)
//     wd_s = (f & 1) ? 0 : wd
//     u   = a + wd_s p                 (decoupled decay, inside the trust ratio as in the paper)
//     W   = |p|_2 over the segment     U = |u|_2 over the segment
//     r   = (f & 2) or W == 0 or U == 0 ?  1  :  W / U
//     p'  = p - (lr r) u
// c1 and c2 are formed in double on the host and rounded to fp32 once.  W, U and r are formed in double from fp64 sums of the
// squares of the fp32 values, and r is rounded to fp32 once.  There is no clamp on W and no gradient clipping.  The fp32
// operation order is fixed with explicit fmaf, contraction is off everywhere else:
//     m'  = fmaf(omb1, g^ - m, m)
//     v'  = fmaf(omb2, fmaf(g^, g^, -v), v)
//     u   = fmaf(wd_s, p, a)
//     p'  = fmaf(-rate_s, u, p)          with rate_s = fl(lr32 * r_s), ONE fp32 product as in LARS's update (sgd.hip)
// sqrtf and / are what the Makefile's flags make of them; no fast-math intrinsic.  (v = g^2 overflows fp32 beyond |g gs| ~ 1e19:
// that is Adam's own limit, not this file's.)
//
// Three launches per step.  lamb_moments_kernel reads p, g, m, v, writes m', v' and the per-unit sums of p^2 and u^2 (24 bytes
// per parameter); lamb_fold_kernel folds them per segment into r; lamb_update_kernel reads p, m', v', RECOMPUTES u through the
// same lamb_u and writes p' (16 bytes per parameter).  Pass 1 leaves p alone, so the norm and the update see the same u bit for
// bit, and no fourth arena-sized buffer is needed.  Nothing is synchronised with the host, no floating-point atomic is used:
// two runs on the same inputs give the same bits.  The fold and the segment cursor are arena.h's; pass 1 says why it is not.
#include "arena.h"

namespace {

struct LambHyper { float omb1, omb2, c1, c2, eps, wd, gscale; };

// the moments of one element; every product that feeds an addition is either an explicit fmaf or kept apart from it
__device__ __forceinline__ void lamb_moments1(float g, float& m, float& v, const LambHyper& h) {
#pragma clang fp contract(off)
    g = g * h.gscale;
    m = fmaf(h.omb1, g - m, m);
    v = fmaf(h.omb2, fmaf(g, g, -v), v);
}

// u of one element from the STORED moments: pass 1 sums its square, pass 3 steps along it -- one function, the same bits
__device__ __forceinline__ float lamb_u(float p, float m, float v, const LambHyper& h) {
#pragma clang fp contract(off)
    const float a = (m * h.c1) / (sqrtf(v * h.c2) + h.eps);
    return fmaf(h.wd, p, a);
}

// ---- pass 1: moments, and per-unit partial sums of p^2 and u^2 ---------------------------------------------------------------------
// arena_walk's units, three arms and visiting order (arena.h) over p, g, m and v, written out: on arena_walk itself this kernel
// compiled to 86 VGPRs for 108 and ran 101.0 us for 96.8 on ResNet-50's arena (profiles/arena_kernels_ab.txt), so it keeps its
// own statement; tests/arena_kernels/test_gpu_kernels.py holds its sums of p^2 to the bits of LARS's.  A full unit is sixteen
// float4 loads issued before the first use; wd_s is one value per block and trip.  p is cacheable and NOT written here (pass 3,
// the bf16 cast and the re-packs read it next); g, m, v are read once and m', v' written once in this pass, and more than the
// Infinity Cache holds passes through before pass 3 reads them back: non-temporal, adam_kernel's choice.  Squares and sums are
// fp64; thread 0 stores the unit's two sums, [p^2, u^2], with one 16-byte vector store.
__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, LambHyper h,
                                                           const int64_t* __restrict__ seg_end,
                                                           const uint8_t* __restrict__ seg_flags,
                                                           const int64_t* __restrict__ seg_first_unit, int nseg, int64_t units,
                                                           f64x2* __restrict__ ws) {
    __shared__ double sh[8];
    const float wd = h.wd;
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        int lo = 0, hi = nseg - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (seg_first_unit[mid] <= u) lo = mid; else hi = mid - 1;
        }
        const int64_t start = lo ? seg_end[lo - 1] : 0;
        const int64_t off = start + (u - seg_first_unit[lo]) * ARENA_UNIT;
        int64_t left = seg_end[lo] - off;
        if (off < start) left = 0;          // (a first_unit table that does not belong to these ends: touch nothing)
        h.wd = (seg_flags[lo] & 1) ? 0.f : wd;
        double sp = 0.0, su = 0.0;
        if (left >= ARENA_UNIT) {
            f32x4 pp[4], gg[4], mm[4], vv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t at = off + (k * 256 + threadIdx.x) * 4;
                pp[k] = ld4(p + at); gg[k] = ldnt4(g + at); mm[k] = ldnt4(m + at); vv[k] = ldnt4(v + at);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float b = mm[k][e], c = vv[k][e];
                    lamb_moments1(gg[k][e], b, c, h);
                    mm[k][e] = b; vv[k][e] = c;
                    const double a = (double)pp[k][e], d = (double)lamb_u(pp[k][e], b, c, h);
                    sp += a * a;
                    su += d * d;
                }
                const int64_t at = off + (k * 256 + threadIdx.x) * 4;
                stnt4(m + at, mm[k]); stnt4(v + at, vv[k]);
            }
        } else if (left > 0) {
            const int len = (int)left, len4 = len & ~3;
            for (int k = threadIdx.x * 4; k < len4; k += 1024) {
                const f32x4 pp = ld4(p + off + k), gg = ldnt4(g + off + k);
                f32x4 mm = ldnt4(m + off + k), vv = ldnt4(v + off + k);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float b = mm[e], c = vv[e];
                    lamb_moments1(gg[e], b, c, h);
                    mm[e] = b; vv[e] = c;
                    const double a = (double)pp[e], d = (double)lamb_u(pp[e], b, c, h);
                    sp += a * a;
                    su += d * d;
                }
                stnt4(m + off + k, mm); stnt4(v + off + k, vv);
            }
            if ((int)threadIdx.x < (len & 3)) {
                const int64_t at = off + len4 + threadIdx.x;
                float b = m[at], c = v[at];
                lamb_moments1(g[at], b, c, h);
                m[at] = b; v[at] = c;
                const double a = (double)p[at], d = (double)lamb_u(p[at], b, c, h);
                sp += a * a;
                su += d * d;
            }
        }
        sp = wave_sum_d(sp);
        su = wave_sum_d(su);
        __syncthreads();            // the previous trip's sh has been read
        if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = sp; sh[4 + (threadIdx.x >> 6)] = su; }
        __syncthreads();
        if (threadIdx.x == 0) {
            f64x2 out;
            out[0] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
            out[1] = ((sh[4] + sh[5]) + sh[6]) + sh[7];
            ws[u] = out;
        }
    }
}

// ---- pass 2: a segment's partials, then the ratio, formed in double and rounded to fp32 once ----------------------------------------
__global__ __launch_bounds__(64) void lamb_fold_kernel(const f64x2* __restrict__ ws, const int64_t* __restrict__ seg_end,
                                                       const int64_t* __restrict__ seg_first_unit,
                                                       const uint8_t* __restrict__ seg_flags, int64_t units,
                                                       float* __restrict__ ratios, double* __restrict__ norms) {
    __shared__ f64x2 sh[64];
    const f64x2 sum = arena_fold_segment(ws, seg_end, seg_first_unit, units, sh);
    if (threadIdx.x != 0) return;
    const int s = blockIdx.x;
    const double W = sqrt(sum[0]), U = sqrt(sum[1]);
    double r = 1.0;
    if (!(seg_flags[s] & 2) && W > 0.0 && U > 0.0) r = W / U;
    ratios[s] = (float)r;
    if (norms) { norms[2 * s] = W; norms[2 * s + 1] = U; }
}

// ---- pass 3: p' = p - (lr r_s) u ------------------------------------------------------------------------------------------------------
// A grid-stride loop behind arena.h's segment cursor, ends, flags and ratios in LDS (8 + 1 + 4 KB).  p cacheable, the moments
// non-temporal (read once, nothing of them is left in the Infinity Cache by now).  u is lamb_u on the stored m', v' and the p pass 1
// saw.
__global__ __launch_bounds__(256) void lamb_update_kernel(float* p, const float* __restrict__ m, const float* __restrict__ v,
                                                          int64_t n, LambHyper h, float lr, const int64_t* __restrict__ seg_end,
                                                          const uint8_t* __restrict__ seg_flags, const float* __restrict__ seg_ratio,
                                                          int nseg) {
    __shared__ int64_t ends[SEG_MAX_SEGMENTS];
    __shared__ float ratio[SEG_MAX_SEGMENTS];
    __shared__ uint8_t flags[SEG_MAX_SEGMENTS];
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    f32x4 pp = {0.f, 0.f, 0.f, 0.f}, mm = pp, vv = pp;
    if (i < n4) { pp = ld4(p + i * 4); mm = ldnt4(m + i * 4); vv = ldnt4(v + i * 4); }
    seg_load(ends, flags, ratio, seg_end, seg_flags, seg_ratio, nseg);
    __syncthreads();
    const float wd = h.wd;
    int seg = i < n4 ? seg_find(ends, nseg, i * 4) : 0;
    while (i < n4) {
        seg = seg_advance(ends, nseg, seg, i * 4);
        h.wd = (flags[seg] & 1) ? 0.f : wd;
        const float rate = lr * ratio[seg];
#pragma unroll
        for (int e = 0; e < 4; ++e) pp[e] = fmaf(-rate, lamb_u(pp[e], mm[e], vv[e], h), pp[e]);
        st4(p + i * 4, pp);
        i += stride;
        if (i < n4) { pp = ld4(p + i * 4); mm = ldnt4(m + i * 4); vv = ldnt4(v + i * 4); }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {         // the last segment's ragged end
        const int64_t t = n4 * 4 + threadIdx.x;
        h.wd = (flags[nseg - 1] & 1) ? 0.f : wd;
        const float rate = lr * ratio[nseg - 1];
        p[t] = fmaf(-rate, lamb_u(p[t], m[t], v[t], h), p[t]);
    }
}

// beta in [0, 1), c >= 1, eps >= 0; a NaN fails every comparison
bool lamb_scalars_ok(double beta1, double beta2, double c1, double c2, double eps) {
    return beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && c1 >= 1.0 && c2 >= 1.0 && eps >= 0.0;
}

}  // namespace

extern "C" int loans_lamb_moments_f32(const float* p, const float* g, float* m, float* v, int64_t n, double beta1, double beta2,
                                      double c1, double c2, double eps, double weight_decay_rate, double grad_scale,
                                      const int64_t* seg_end_dev, const uint8_t* seg_flags_dev, const int64_t* seg_first_unit_dev,
                                      const int64_t* seg_end_host, int32_t nseg, void* workspace, int64_t workspace_bytes,
                                      void* stream) {
    if (!p || !g || !m || !v || n <= 0 || !seg_end_dev || !seg_flags_dev || !seg_first_unit_dev || !seg_end_host || !workspace)
        return LOANS_EINVAL;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)workspace) & 15) ||
        (((uintptr_t)seg_end_dev | (uintptr_t)seg_first_unit_dev) & 7))
        return LOANS_EINVAL;
    if (!lamb_scalars_ok(beta1, beta2, c1, c2, eps)) return LOANS_EINVAL;
    const int64_t units = seg_table_units(seg_end_host, nseg, n, ARENA_UNIT);
    if (units < 0 || workspace_bytes < units * (int64_t)sizeof(f64x2)) return LOANS_EINVAL;
    LambHyper h;
    h.omb1 = (float)(1.0 - beta1); h.omb2 = (float)(1.0 - beta2); h.c1 = (float)c1; h.c2 = (float)c2; h.eps = (float)eps;
    h.wd = (float)weight_decay_rate; h.gscale = (float)grad_scale;
    hipLaunchKernelGGL(lamb_moments_kernel, dim3(grid_for(units, 1)), dim3(256), 0, as_stream(stream), p, g, m, v, h, seg_end_dev,
                       seg_flags_dev, seg_first_unit_dev, nseg, units, static_cast<f64x2*>(workspace));
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_lamb_ratios_f32(int64_t n, const int64_t* seg_end_dev, const uint8_t* seg_flags_dev,
                                     const int64_t* seg_first_unit_dev, const int64_t* seg_end_host, int32_t nseg,
                                     float* ratios_dev, double* norms_dev, const void* workspace, int64_t workspace_bytes,
                                     void* stream) {
    if (n <= 0 || !seg_end_dev || !seg_flags_dev || !seg_first_unit_dev || !seg_end_host || !ratios_dev || !workspace)
        return LOANS_EINVAL;
    if (((uintptr_t)workspace & 15) || (((uintptr_t)seg_end_dev | (uintptr_t)seg_first_unit_dev | (uintptr_t)norms_dev) & 7) ||
        ((uintptr_t)ratios_dev & 3))
        return LOANS_EINVAL;
    const int64_t units = seg_table_units(seg_end_host, nseg, n, ARENA_UNIT);
    if (units < 0 || workspace_bytes < units * (int64_t)sizeof(f64x2)) return LOANS_EINVAL;
    hipLaunchKernelGGL(lamb_fold_kernel, dim3(nseg), dim3(64), 0, as_stream(stream), static_cast<const f64x2*>(workspace),
                       seg_end_dev, seg_first_unit_dev, seg_flags_dev, units, ratios_dev, norms_dev);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_lamb_update_f32(float* p, const float* m, const float* v, int64_t n, double lr, double c1, double c2,
                                     double eps, double weight_decay_rate, const int64_t* seg_end_dev,
                                     const uint8_t* seg_flags_dev, const float* ratios_dev, const int64_t* seg_end_host,
                                     int32_t nseg, void* stream) {
    if (!p || !m || !v || n <= 0 || !seg_end_dev || !seg_flags_dev || !ratios_dev || !seg_end_host) return LOANS_EINVAL;
    if ((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) || ((uintptr_t)seg_end_dev & 7) || ((uintptr_t)ratios_dev & 3))
        return LOANS_EINVAL;
    if (!lamb_scalars_ok(0.0, 0.0, c1, c2, eps)) return LOANS_EINVAL;
    if (seg_table_units(seg_end_host, nseg, n, ARENA_UNIT) < 0) return LOANS_EINVAL;
    LambHyper h;
    h.omb1 = 0.f; h.omb2 = 0.f; h.c1 = (float)c1; h.c2 = (float)c2; h.eps = (float)eps; h.wd = (float)weight_decay_rate;
    h.gscale = 0.f;
    hipLaunchKernelGGL(lamb_update_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, as_stream(stream), p, m, v, n, h,
                       (float)lr, seg_end_dev, seg_flags_dev, ratios_dev, nseg);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}
