// Momentum SGD over the flat parameter arena (Chainer 4.1 MomentumSGDRule, the WeightDecay hook applied to the gradient first): plain,
// with per-segment weight decay, and LARS (You et al. 2017), whose rate is scaled per segment by the trust ratio
//   r_s = eta * |p_s| / (|g_s| + wd_s * |p_s| + eps)
// LARS is two passes.  lars_partials_kernel + lars_fold_kernel read p and g once and leave one ratio per segment in device memory;
// the update is the segmented momentum SGD kernel with that table beside `ends` and `flags` in LDS.  Nothing is synchronised with
// the host, no floating-point atomic is used: two runs on the same inputs give the same bits.  The pieces are arena.h's.
#include "arena.h"

namespace {

struct SgdHyper { float lr, momentum, wd, gscale; };

__device__ __forceinline__ void sgd1(float& p, float g, float& v, const SgdHyper& h) {
    g = g * h.gscale + h.wd * p;
    v = h.momentum * v - h.lr * g;
    p += v;
}

// the structure of adam_kernel: g read once, v read and written once per step -- non-temporal; p stays cacheable for the same
// reason as there (the bf16 cast and the re-packs of the next step read it).  20 bytes per parameter against plain Adam's 28.
__global__ __launch_bounds__(256) void momentum_sgd_kernel(float* p, const float* g, float* v, int64_t n, SgdHyper h,
                                                           const float* lr_dev) {
    if (lr_dev) h.lr = *lr_dev;         // read from device memory: the launch can live in a hipGraph
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 pp = ld4(p + i * 4), gg = ldnt4(g + i * 4), vv = ldnt4(v + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a = pp[e], b = vv[e];
            sgd1(a, gg[e], b, h);
            pp[e] = a; vv[e] = b;
        }
        st4(p + i * 4, pp); stnt4(v + i * 4, vv);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = n4 * 4 + threadIdx.x;
        sgd1(p[i], g[i], v[i], h);
    }
}

// ---- with per-segment weight decay, and per-segment rate where RATIO ------------------------------------------------------------
// momentum_sgd_kernel with h.wd replaced by 0 inside the segments whose flag has bit 0 set (BN gamma / beta, biases), behind
// arena.h's segment cursor; p cacheable, v and g non-temporal as there.  RATIO (LARS's update): the ratio table sits in LDS beside
// ends and flags (8 + 1 + 4 KB) and, per segment, h.lr = fl(lr32 * r_s): ONE fp32 product of the rate as the kernel holds it.
// Without RATIO there is no ratio array and no product.
template <bool RATIO>
__global__ __launch_bounds__(256) void momentum_sgd_seg_kernel(float* p, const float* g, float* v, int64_t n, SgdHyper h,
                                                               const float* lr_dev, const int64_t* __restrict__ seg_end,
                                                               const uint8_t* __restrict__ seg_flags,
                                                               const float* __restrict__ seg_ratio, int nseg) {
    __shared__ int64_t ends[SEG_MAX_SEGMENTS];
    __shared__ float ratio[RATIO ? SEG_MAX_SEGMENTS : 1];
    __shared__ uint8_t flags[SEG_MAX_SEGMENTS];
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    f32x4 pp = {0.f, 0.f, 0.f, 0.f}, gg = pp, vv = pp;
    if (i < n4) { pp = ld4(p + i * 4); gg = ldnt4(g + i * 4); vv = ldnt4(v + i * 4); }
    seg_load(ends, flags, RATIO ? ratio : nullptr, seg_end, seg_flags, seg_ratio, nseg);
    if (lr_dev) h.lr = *lr_dev;
    __syncthreads();
    const float wd = h.wd, lr = h.lr;
    auto hyper_of = [&](int seg) {
        h.wd = (flags[seg] & 1) ? 0.f : wd;
        if (RATIO) h.lr = lr * ratio[seg];
    };
    int seg = i < n4 ? seg_find(ends, nseg, i * 4) : 0;
    while (i < n4) {
        seg = seg_advance(ends, nseg, seg, i * 4);
        hyper_of(seg);
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
        hyper_of(nseg - 1);
        sgd1(p[t], g[t], v[t], h);
    }
}

// ---- LARS, norms: per-unit partial sums of squares --------------------------------------------------------------------------------
// arena.h's unit walk over p and g.  g is read once per step: non-temporal; p stays cacheable for the reason given at adam_kernel
// -- the update, the bf16 cast and the re-packs read it next.  Every element is converted to double, squared and accumulated in
// double: the square of an fp32 value is exact in fp64, only the additions round, 1e-25 does not vanish and 1e25 does not
// overflow.  The kernel is HBM-bound, the fp64 FMAs are hidden.  ws[u] = [the sum of p^2, of g^2].
__global__ __launch_bounds__(256) void lars_partials_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                            const int64_t* __restrict__ seg_end,
                                                            const int64_t* __restrict__ seg_first_unit, int nseg, int64_t units,
                                                            f64x2* __restrict__ ws) {
    __shared__ double sh[8];
    float* const buf[1] = {const_cast<float*>(g)};
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const ArenaUnit at = arena_unit(seg_end, seg_first_unit, nseg, u);
        double s[2] = {0.0, 0.0};
        arena_walk(p, buf, 0u, at.off, at.left, [&](float pe, float (&x)[1]) {
            const double a = (double)pe, b = (double)x[0];
            s[0] += a * a;
            s[1] += b * b;
        });
        arena_block_sums(s, sh, reinterpret_cast<double*>(ws + u));
    }
}

// ---- LARS, fold: a segment's partials, then the ratio, formed in double and rounded to fp32 once -----------------------------------
struct LarsHyper { double wd, gscale_abs, eta, eps; };

__global__ __launch_bounds__(64) void lars_fold_kernel(const f64x2* __restrict__ ws, const int64_t* __restrict__ seg_end,
                                                       const int64_t* __restrict__ seg_first_unit,
                                                       const uint8_t* __restrict__ seg_flags, int64_t units, LarsHyper h,
                                                       float* __restrict__ ratios, double* __restrict__ norms) {
    __shared__ f64x2 sh[64];
    const f64x2 sum = arena_fold_segment(ws, seg_end, seg_first_unit, units, sh);
    if (threadIdx.x != 0) return;
    const int s = blockIdx.x;
    const uint8_t f = seg_flags[s];
    const double W = sqrt(sum[0]), G = h.gscale_abs * sqrt(sum[1]);
    const double wd = (f & 1) ? 0.0 : h.wd;
    double r = 1.0;
    if (!(f & 2) && W > 0.0 && G > 0.0) r = h.eta * W / (G + wd * W + h.eps);
    ratios[s] = (float)r;
    if (norms) { norms[2 * s] = W; norms[2 * s + 1] = G; }
}

SgdHyper sgd_hyper(double lr, double momentum, double weight_decay_rate, double grad_scale) {
    SgdHyper h;
    h.lr = (float)lr; h.momentum = (float)momentum; h.wd = (float)weight_decay_rate; h.gscale = (float)grad_scale;
    return h;
}

}  // namespace

extern "C" int loans_momentum_sgd_f32(float* p, const float* g, float* v, int64_t n, double lr, const float* lr_dev,
                                      double momentum, double weight_decay_rate, double grad_scale, void* stream) {
    if (!p || !g || !v || n <= 0) return LOANS_EINVAL;
    hipLaunchKernelGGL(momentum_sgd_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, as_stream(stream), p, g, v, n,
                       sgd_hyper(lr, momentum, weight_decay_rate, grad_scale), lr_dev);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_momentum_sgd_seg_f32(float* p, const float* g, float* v, int64_t n, double lr, const float* lr_dev, double momentum,
                                          double weight_decay_rate, double grad_scale, const int64_t* seg_end_dev,
                                          const uint8_t* seg_flags_dev, const int64_t* seg_end_host, int32_t nseg, void* stream) {
    if (!p || !g || !v || n <= 0 || !seg_end_dev || !seg_flags_dev || !seg_end_host) return LOANS_EINVAL;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)v) & 15) || ((uintptr_t)seg_end_dev & 7)) return LOANS_EINVAL;
    if (seg_table_units(seg_end_host, nseg, n, ARENA_UNIT) < 0) return LOANS_EINVAL;
    hipLaunchKernelGGL(momentum_sgd_seg_kernel<false>, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, as_stream(stream), p, g, v, n,
                       sgd_hyper(lr, momentum, weight_decay_rate, grad_scale), lr_dev, seg_end_dev, seg_flags_dev,
                       (const float*)nullptr, nseg);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_momentum_sgd_max_segments(void) { return SEG_MAX_SEGMENTS; }

extern "C" int64_t loans_lars_workspace_bytes(const int64_t* seg_end_host, int32_t nseg) {
    const int64_t units = seg_table_units(seg_end_host, nseg, -1, ARENA_UNIT);
    return units < 0 ? -1 : units * (int64_t)sizeof(f64x2);
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
    const int64_t units = seg_table_units(seg_end_host, nseg, n, ARENA_UNIT);
    if (units < 0 || workspace_bytes < units * (int64_t)sizeof(f64x2)) return LOANS_EINVAL;
    LarsHyper h;
    h.wd = weight_decay_rate; h.gscale_abs = grad_scale < 0.0 ? -grad_scale : grad_scale; h.eta = eta; h.eps = eps;
    f64x2* ws = static_cast<f64x2*>(workspace);
    hipLaunchKernelGGL(lars_partials_kernel, dim3(grid_for(units, 1)), dim3(256), 0, as_stream(stream), p, g, seg_end_dev,
                       seg_first_unit_dev, nseg, units, ws);
    LOANS_LAUNCH_CHECK();
    hipLaunchKernelGGL(lars_fold_kernel, dim3(nseg), dim3(64), 0, as_stream(stream), ws, seg_end_dev, seg_first_unit_dev,
                       seg_flags_dev, units, h, ratios_dev, norms_dev);
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
    if (seg_table_units(seg_end_host, nseg, n, ARENA_UNIT) < 0) return LOANS_EINVAL;
    hipLaunchKernelGGL(momentum_sgd_seg_kernel<true>, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, as_stream(stream), p, g, v, n,
                       sgd_hyper(lr, momentum, weight_decay_rate, grad_scale), lr_dev, seg_end_dev, seg_flags_dev, ratios_dev, nseg);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}
