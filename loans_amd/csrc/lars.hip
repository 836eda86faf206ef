// LARS (You et al. 2017) over the flat parameter arena: momentum SGD whose rate is scaled per segment by the trust ratio
//   r_s = eta * |p_s| / (|g_s| + wd_s * |p_s| + eps)
// Two passes.  lars_partials_kernel + lars_fold_kernel read p and g once and leave one ratio per segment in device memory;
// lars_update_kernel is momentum_sgd_seg_kernel (misc.hip) with that table beside `ends` and `flags` in LDS.  Nothing is
// synchronised with the host, no floating-point atomic is used: two runs on the same inputs give the same bits.
#include "common.h"

namespace {

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ f32x4 ldnt4(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); }
__device__ __forceinline__ void stnt4(float* p, f32x4 v) { __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p)); }

constexpr int LARS_UNIT = LOANS_LARS_UNIT;
constexpr int LARS_MAX_SEGMENTS = LOANS_LARS_MAX_SEGMENTS;

// ---- norms: per-unit partial sums of squares --------------------------------------------------------------------------------------
// Work is cut into units of LARS_UNIT floats PER SEGMENT, as average_jobs_kernel cuts its jobs: unit u belongs to the segment with
// the largest first_unit <= u (u is the same for the whole block: scalar loads), so a unit never straddles a boundary.  A full unit
// is four float4 of p and of g per thread, all eight loads issued before the first use; a segment's last, short unit takes float4
// while they fit and single floats for the n & 3 behind them (only the last segment can have those).  g is read once per step:
// non-temporal; p stays cacheable for the reason given at adam_kernel -- the update, the bf16 cast and the re-packs read it next.
// Every element is converted to double, squared and accumulated in double: the square of an fp32 value is exact in fp64, only the
// additions round, 1e-25 does not vanish and 1e25 does not overflow.  The kernel is HBM-bound, the fp64 FMAs are hidden.
// Order of the additions, fixed: a thread's elements (float4 k ascending, lane e ascending), the xor butterfly 32, 16 .. 1 inside
// the wave, waves 0..3 through LDS.  Thread 0 stores the unit's two sums as one 16-byte vector store to ws[u].
typedef double LarsPartial __attribute__((ext_vector_type(2)));     // [0] the sum of p^2, [1] of g^2

__global__ __launch_bounds__(256) void lars_partials_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                            const int64_t* __restrict__ seg_end,
                                                            const int64_t* __restrict__ seg_first_unit, int nseg, int64_t units,
                                                            LarsPartial* __restrict__ ws) {
    __shared__ double sh[8];
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        int lo = 0, hi = nseg - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (seg_first_unit[mid] <= u) lo = mid; else hi = mid - 1;
        }
        const int64_t start = lo ? seg_end[lo - 1] : 0;
        const int64_t off = start + (u - seg_first_unit[lo]) * LARS_UNIT;
        int64_t left = seg_end[lo] - off;
        if (off < start) left = 0;          // (a first_unit table that does not belong to these ends: read nothing)
        double sp = 0.0, sg = 0.0;
        if (left >= LARS_UNIT) {
            f32x4 pp[4], gg[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { pp[k] = ld4(p + off + (k * 256 + threadIdx.x) * 4); gg[k] = ldnt4(g + off + (k * 256 + threadIdx.x) * 4); }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double a = (double)pp[k][e], b = (double)gg[k][e];
                    sp += a * a;
                    sg += b * b;
                }
            }
        } else if (left > 0) {
            const int m = (int)left, m4 = m & ~3;
            for (int k = threadIdx.x * 4; k < m4; k += 1024) {
                const f32x4 pp = ld4(p + off + k), gg = ldnt4(g + off + k);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double a = (double)pp[e], b = (double)gg[e];
                    sp += a * a;
                    sg += b * b;
                }
            }
            if ((int)threadIdx.x < (m & 3)) {
                const double a = (double)p[off + m4 + threadIdx.x], b = (double)g[off + m4 + threadIdx.x];
                sp += a * a;
                sg += b * b;
            }
        }
        sp = wave_sum_d(sp);
        sg = wave_sum_d(sg);
        __syncthreads();            // the previous trip's sh has been read
        if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = sp; sh[4 + (threadIdx.x >> 6)] = sg; }
        __syncthreads();
        if (threadIdx.x == 0) {
            LarsPartial out;
            out[0] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
            out[1] = ((sh[4] + sh[5]) + sh[6]) + sh[7];
            ws[u] = out;
        }
    }
}

// ---- fold: a segment's partials in ascending unit order, then the ratio, formed in double and rounded to fp32 once -------------------
// One wave per segment.  The order of the additions is the units' -- one chain per sum --, but the loads are not on that chain: the
// wave fetches 64 partials at a time, one 16-byte load per lane, the next 64 before the current ones are added, and passes them
// through LDS to an unrolled loop.  (One thread per segment walking its partials alone waits for every load, 576 round trips for
// ResNet-50's largest tensor: the two launches took 154 us that way, profiles/imagenet_lars.txt.)
struct LarsHyper { double wd, gscale_abs, eta, eps; };

__global__ __launch_bounds__(64) void lars_fold_kernel(const LarsPartial* __restrict__ ws, const int64_t* __restrict__ seg_end,
                                                       const int64_t* __restrict__ seg_first_unit,
                                                       const uint8_t* __restrict__ seg_flags, int nseg, int64_t units, LarsHyper h,
                                                       float* __restrict__ ratios, double* __restrict__ norms) {
    __shared__ LarsPartial sh[64];
    const int s = blockIdx.x, lane = threadIdx.x;
    const int64_t start = s ? seg_end[s - 1] : 0;
    const int64_t first = seg_first_unit[s];
    int64_t count = (seg_end[s] - start + LARS_UNIT - 1) / LARS_UNIT;
    if (first < 0 || first + count > units) count = 0;          // (a first_unit table that does not belong to these ends)
    const LarsPartial zero = {0.0, 0.0};
    double sp = 0.0, sg = 0.0;
    LarsPartial next = lane < count ? ws[first + lane] : zero;
    for (int64_t base = 0; base < count; base += 64) {
        sh[lane] = next;
        next = base + 64 + lane < count ? ws[first + base + 64 + lane] : zero;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 64; ++k) {          // every lane carries the same chain (broadcast reads, no divergence); slots behind the
            sp += sh[k][0];                     // segment's last unit hold +0.0, which changes no bit of a non-negative sum
            sg += sh[k][1];
        }
        __syncthreads();
    }
    if (lane != 0) return;
    const uint8_t f = seg_flags[s];
    const double W = sqrt(sp), G = h.gscale_abs * sqrt(sg);
    const double wd = (f & 1) ? 0.0 : h.wd;
    double r = 1.0;
    if (!(f & 2) && W > 0.0 && G > 0.0) r = h.eta * W / (G + wd * W + h.eps);
    ratios[s] = (float)r;
    if (norms) { norms[2 * s] = W; norms[2 * s + 1] = G; }
}

// ---- update -----------------------------------------------------------------------------------------------------------------------
// momentum_sgd_seg_kernel of misc.hip, its structure kept -- the first trip's loads go out before the table is fetched, a thread
// bisects once and carries a forward-only cursor, p cacheable, v and g non-temporal -- with the ratio table in LDS beside ends and
// flags (8 + 1 + 4 KB) and, per segment, h.lr = fl(lr32 * r_s): ONE fp32 product of the rate as the kernel holds it.  sgd1 is
// misc.hip's, restated: same source, same flags.
struct SgdHyper { float lr, momentum, wd, gscale; };

__device__ __forceinline__ void sgd1(float& p, float g, float& v, const SgdHyper& h) {
    g = g * h.gscale + h.wd * p;
    v = h.momentum * v - h.lr * g;
    p += v;
}

__global__ __launch_bounds__(256) void lars_update_kernel(float* p, const float* g, float* v, int64_t n, SgdHyper h,
                                                          const float* lr_dev, const int64_t* __restrict__ seg_end,
                                                          const uint8_t* __restrict__ seg_flags, const float* __restrict__ seg_ratio,
                                                          int nseg) {
    __shared__ int64_t ends[LARS_MAX_SEGMENTS];
    __shared__ float ratio[LARS_MAX_SEGMENTS];
    __shared__ uint8_t flags[LARS_MAX_SEGMENTS];
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    f32x4 pp = {0.f, 0.f, 0.f, 0.f}, gg = pp, vv = pp;
    if (i < n4) { pp = ld4(p + i * 4); gg = ldnt4(g + i * 4); vv = ldnt4(v + i * 4); }
    for (int s = threadIdx.x; s < nseg; s += 256) { ends[s] = seg_end[s]; flags[s] = seg_flags[s]; ratio[s] = seg_ratio[s]; }
    if (lr_dev) h.lr = *lr_dev;
    __syncthreads();
    const float wd = h.wd, lr = h.lr;
    int seg = 0;
    if (i < n4) {           // the first segment whose end lies behind float i * 4
        int lo = 0, hi = nseg - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ends[mid] > i * 4) hi = mid; else lo = mid + 1;
        }
        seg = lo;
    }
    while (i < n4) {
        while (seg < nseg - 1 && ends[seg] <= i * 4) ++seg;         // (the last end is n > i * 4)
        h.wd = (flags[seg] & 1) ? 0.f : wd;
        h.lr = lr * ratio[seg];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a = pp[e], b = vv[e];
            sgd1(a, gg[e], b, h);
            pp[e] = a; vv[e] = b;
        }
        st4(p + i * 4, pp); stnt4(v + i * 4, vv);
        i += stride;
        if (i < n4) { pp = ld4(p + i * 4); gg = ldnt4(g + i * 4); vv = ldnt4(v + i * 4); }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {         // the last segment's ragged end
        const int64_t t = n4 * 4 + threadIdx.x;
        h.wd = (flags[nseg - 1] & 1) ? 0.f : wd;
        h.lr = lr * ratio[nseg - 1];
        sgd1(p[t], g[t], v[t], h);
    }
}

// ascending, no empty segment, float4-aligned boundaries, the last one at n; the number of units, or -1
int64_t lars_units(const int64_t* seg_end_host, int32_t nseg, int64_t n) {
    if (!seg_end_host || nseg <= 0 || nseg > LARS_MAX_SEGMENTS) return -1;
    int64_t prev = 0, units = 0;
    for (int s = 0; s < nseg; ++s) {
        const int64_t e = seg_end_host[s];
        if (e <= prev || (s < nseg - 1 && (e & 3))) return -1;
        units += (e - prev + LARS_UNIT - 1) / LARS_UNIT;
        prev = e;
    }
    if (n >= 0 && prev != n) return -1;
    return units;
}

}  // namespace

extern "C" int64_t loans_lars_workspace_bytes(const int64_t* seg_end_host, int32_t nseg) {
    const int64_t units = lars_units(seg_end_host, nseg, -1);
    return units < 0 ? -1 : units * (int64_t)sizeof(LarsPartial);
}

extern "C" int loans_lars_ratios_f32(const float* p, const float* g, int64_t n, double weight_decay_rate, double grad_scale,
                                     double eta, double eps, const int64_t* seg_end_dev, const uint8_t* seg_flags_dev,
                                     const int64_t* seg_first_unit_dev, const int64_t* seg_end_host, int32_t nseg, float* ratios_dev,
                                     double* norms_dev, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!p || !g || n <= 0 || !seg_end_dev || !seg_flags_dev || !seg_first_unit_dev || !seg_end_host || !ratios_dev || !workspace)
        return LOANS_EINVAL;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)workspace) & 15) || (((uintptr_t)seg_end_dev | (uintptr_t)seg_first_unit_dev) & 7) ||
        ((uintptr_t)ratios_dev & 3) || ((uintptr_t)norms_dev & 7))
        return LOANS_EINVAL;
    if (!(eta > 0.0) || !(eps >= 0.0)) return LOANS_EINVAL;
    const int64_t units = lars_units(seg_end_host, nseg, n);
    if (units < 0 || workspace_bytes < units * (int64_t)sizeof(LarsPartial)) return LOANS_EINVAL;
    LarsHyper h;
    h.wd = weight_decay_rate; h.gscale_abs = grad_scale < 0.0 ? -grad_scale : grad_scale; h.eta = eta; h.eps = eps;
    LarsPartial* ws = static_cast<LarsPartial*>(workspace);
    hipLaunchKernelGGL(lars_partials_kernel, dim3(grid_for(units, 1)), dim3(256), 0, as_stream(stream), p, g, seg_end_dev,
                       seg_first_unit_dev, nseg, units, ws);
    LOANS_LAUNCH_CHECK();
    hipLaunchKernelGGL(lars_fold_kernel, dim3(nseg), dim3(64), 0, as_stream(stream), ws, seg_end_dev, seg_first_unit_dev,
                       seg_flags_dev, nseg, units, h, ratios_dev, norms_dev);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_lars_update_f32(float* p, const float* g, float* v, int64_t n, double lr, const float* lr_dev, double momentum,
                                     double weight_decay_rate, double grad_scale, const int64_t* seg_end_dev,
                                     const uint8_t* seg_flags_dev, const float* ratios_dev, const int64_t* seg_end_host, int32_t nseg,
                                     void* stream) {
    if (!p || !g || !v || n <= 0 || !seg_end_dev || !seg_flags_dev || !ratios_dev || !seg_end_host) return LOANS_EINVAL;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)v) & 15) || ((uintptr_t)seg_end_dev & 7) || ((uintptr_t)ratios_dev & 3))
        return LOANS_EINVAL;
    if (lars_units(seg_end_host, nseg, n) < 0) return LOANS_EINVAL;
    SgdHyper h;
    h.lr = (float)lr; h.momentum = (float)momentum; h.wd = (float)weight_decay_rate; h.gscale = (float)grad_scale;
    hipLaunchKernelGGL(lars_update_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, as_stream(stream), p, g, v, n, h, lr_dev,
                       seg_end_dev, seg_flags_dev, ratios_dev, nseg);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}
