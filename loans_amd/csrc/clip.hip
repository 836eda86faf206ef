// Gradient clipping by the global L2 norm (Pascanu et al. 2013; chainer.optimizer_hooks.GradientClipping) over the flat gradient
// arena.  For the first n floats g, the optimiser's grad_scale gs and the threshold c > 0:
//   S    = sum g_i^2                      every g_i converted to double and squared (exact), summed in fp64 in a FIXED order
//   N    = |gs| * sqrt(S)                 in double: the norm of the gradient the optimiser will actually apply
//   k    = (N is finite and N > c) ? c / N : 1          in double, rounded to fp32 ONCE
//   g_i' = fl32(g_i * k)                  one fp32 product per element, in place -- skipped entirely when k == 1
// N (rounded to fp32 once) and k are left in a device record of two floats; nothing returns to the host.  N == c does not clip
// (Chainer's `rate < 1`), an all-zero gradient gives N = 0, k = 1 and no division, a non-finite N (a NaN or inf anywhere in g, or
// a sum that overflows) gives k = 1 and leaves g bit for bit as it was, with the non-finite N in the record -- Chainer would write
// 0 * inf there.  c = +inf means "measure only".
// Three launches: grad_sumsq_kernel (one pass over g, one fp64 partial per unit of 4096 floats), grad_clip_fold_kernel (one wave:
// partials -> N, k), grad_scale_dev_kernel (g *= k, or nothing).  No atomic, nothing synchronised with the host: two runs on the same
// inputs give the same bits.
#include "arena.h"

namespace {

constexpr int64_t CLIP_MAX_N = LOANS_GRAD_CLIP_MAX_N;

// ---- pass 1: per-unit partial sums of squares -------------------------------------------------------------------------------------
// arena_walk's three arms and visiting order (arena.h) over g alone, without a segment table: unit u is floats [4096 u,
// min(n, 4096 (u + 1))), the partial of a unit lands in ws[u] whichever block summed it, so the result does not depend on the grid.
// tests/arena_kernels/test_gpu_kernels.py holds the two walks to one order.  g is read non-temporally: the clipped copy, if any,
// is written by the third launch from a second read.  Every element is converted to double and squared -- exact, 24 + 24 bits in
// 53 --, only the additions round; 1e-25 does not vanish and 1e25 does not overflow.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n, int64_t units,
                                                         double* __restrict__ ws) {
    __shared__ double sh[4];
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int64_t off = u * ARENA_UNIT;
        const int64_t left = n - off;
        double s[1] = {0.0};
        auto sum4 = [&](f32x4 gg) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double a = (double)gg[e];
                s[0] += a * a;
            }
        };
        if (left >= ARENA_UNIT) {
            f32x4 gg[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) gg[k] = ldnt4(g + off + (k * 256 + threadIdx.x) * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) sum4(gg[k]);
        } else if (left > 0) {
            const int m = (int)left, m4 = m & ~3;
            for (int k = threadIdx.x * 4; k < m4; k += 1024) sum4(ldnt4(g + off + k));
            if ((int)threadIdx.x < (m & 3)) {
                const double a = (double)g[off + m4 + threadIdx.x];
                s[0] += a * a;
            }
        }
        arena_block_sums(s, sh, ws + u);
    }
}

// ---- pass 2: the partials -> N and k ----------------------------------------------------------------------------------------------
// One wave.  A single chain over the partials, as arena_fold_segment walks a segment's, puts one dependent fp64 addition per unit on
// the critical path (576 units: 14 to 17 us there) and ResNet-50's arena is ~6.3 k units, so this is a tree: lane l sums partials
// l, l + 64, l + 128, .. in ascending order -- ceil(units / 64) additions deep -- and the 64 lane sums meet in the xor butterfly.
// The loads are not on that chain: a lane fetches FOLD_BATCH of its partials at a time, all of them in flight together, and the next
// batch before the current one is added.  (With one fetch ahead every addition waited for a round trip to memory: 98 of them,
// 27 us for ResNet-50, profiles/imagenet_clip.txt.)  The order is a pure function of n.  A slot behind the last partial holds +0.0,
// which changes no bit of a non-negative sum.  N, k are formed in double and each rounded to fp32 once; lane 0 stores them as one
// 8-byte vector store.
typedef float ClipRecord __attribute__((ext_vector_type(2)));       // [0] = N, [1] = k
constexpr int FOLD_BATCH = 32;

__global__ __launch_bounds__(64) void grad_clip_fold_kernel(const double* __restrict__ ws, int64_t units, double gscale_abs,
                                                            double max_norm, ClipRecord* __restrict__ record) {
    const int lane = threadIdx.x;
    double s = 0.0;
    double cur[FOLD_BATCH], next[FOLD_BATCH];
#pragma unroll
    for (int j = 0; j < FOLD_BATCH; ++j) {
        const int64_t i = (int64_t)j * 64 + lane;
        next[j] = i < units ? ws[i] : 0.0;
    }
    for (int64_t base = 0; base < units; base += FOLD_BATCH * 64) {
#pragma unroll
        for (int j = 0; j < FOLD_BATCH; ++j) cur[j] = next[j];
#pragma unroll
        for (int j = 0; j < FOLD_BATCH; ++j) {          // the next batch: FOLD_BATCH independent loads in flight
            const int64_t i = base + (int64_t)(FOLD_BATCH + j) * 64 + lane;
            next[j] = i < units ? ws[i] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < FOLD_BATCH; ++j) s += cur[j];       // ascending: partials base + 64 j + lane
    }
    s = wave_sum_d(s);
    if (lane != 0) return;
    const double N = gscale_abs * sqrt(s);
    double k = 1.0;
    if (N <= 1.7976931348623157e308 && N > max_norm) k = max_norm / N;         // (a NaN fails both comparisons)
    ClipRecord out;
    out[0] = (float)N;
    out[1] = (float)k;
    *record = out;
}

// ---- pass 3: g *= k, in place, or nothing -----------------------------------------------------------------------------------------
// Every block reads k from the record -- the same address for all threads: a scalar load -- and returns before touching g if it
// is exactly 1: a step that does not clip costs this launch and no traffic.  Otherwise one fp32 product per element, float4 grid
// stride, the n & 3 floats behind them by block 0.  Cache hints, NT_LOAD / NT_STORE: the optimiser's kernel reads g next, so the
// store stays cacheable (the arena fits in the Infinity Cache) and so does the load; tools/clip_bench.py --exp times all four arms
// (profiles/imagenet_clip.txt).
template <bool NT_LOAD, bool NT_STORE>
__global__ __launch_bounds__(256) void grad_scale_dev_kernel(float* __restrict__ g, int64_t n, const float* __restrict__ record) {
    const float k = record[1];
    if (k == 1.0f) return;
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        f32x4 v = NT_LOAD ? ldnt4(g + i * 4) : ld4(g + i * 4);
        v *= k;
        if (NT_STORE) stnt4(g + i * 4, v); else st4(g + i * 4, v);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) g[n4 * 4 + threadIdx.x] *= k;
}

constexpr int CLIP_HINT = 0;        // bit 0: non-temporal load, bit 1: non-temporal store -- the arm that won the measurement

int clip_hint() {
#ifdef LOANS_EXPERIMENT
    const char* e = getenv("LOANS_CLIP_HINT");      // read on every call: the bench interleaves the arms in one process
    if (e && *e) return atoi(e) & 3;
#endif
    return CLIP_HINT;
}

inline int64_t clip_units(int64_t n) { return (n + ARENA_UNIT - 1) / ARENA_UNIT; }

}  // namespace

extern "C" int64_t loans_grad_clip_workspace_bytes(int64_t n) {
    if (n <= 0) return LOANS_EINVAL;
    if (n > CLIP_MAX_N) return LOANS_ERANGE;
    return clip_units(n) * (int64_t)sizeof(double);
}

extern "C" int loans_grad_norm_f32(const float* g, int64_t n, double grad_scale, double max_norm, void* workspace,
                                   int64_t workspace_bytes, float* record_dev, void* stream) {
    if (!g || !workspace || !record_dev || n <= 0) return LOANS_EINVAL;
    if ((((uintptr_t)g | (uintptr_t)workspace) & 15) || ((uintptr_t)record_dev & 7)) return LOANS_EINVAL;
    if (!(max_norm > 0.0)) return LOANS_EINVAL;                                         // (NaN fails the comparison)
    if (!(grad_scale >= -1.7976931348623157e308 && grad_scale <= 1.7976931348623157e308)) return LOANS_EINVAL;
    if (n > CLIP_MAX_N) return LOANS_ERANGE;
    const int64_t units = clip_units(n);
    if (workspace_bytes < units * (int64_t)sizeof(double)) return LOANS_EINVAL;
    double* ws = static_cast<double*>(workspace);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(grid_for(units, 1)), dim3(256), 0, as_stream(stream), g, n, units, ws);
    LOANS_LAUNCH_CHECK();
    hipLaunchKernelGGL(grad_clip_fold_kernel, dim3(1), dim3(64), 0, as_stream(stream), ws, units,
                       grad_scale < 0.0 ? -grad_scale : grad_scale, max_norm, reinterpret_cast<ClipRecord*>(record_dev));
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_grad_clip_apply_f32(float* g, int64_t n, const float* record_dev, void* stream) {
    if (!g || !record_dev || n <= 0) return LOANS_EINVAL;
    if (((uintptr_t)g & 15) || ((uintptr_t)record_dev & 7)) return LOANS_EINVAL;
    if (n > CLIP_MAX_N) return LOANS_ERANGE;
    const dim3 grid(grid_for((n + 3) / 4, 256)), block(256);
    switch (clip_hint()) {
    case 0: hipLaunchKernelGGL((grad_scale_dev_kernel<false, false>), grid, block, 0, as_stream(stream), g, n, record_dev); break;
    case 1: hipLaunchKernelGGL((grad_scale_dev_kernel<true, false>), grid, block, 0, as_stream(stream), g, n, record_dev); break;
    case 2: hipLaunchKernelGGL((grad_scale_dev_kernel<false, true>), grid, block, 0, as_stream(stream), g, n, record_dev); break;
    default: hipLaunchKernelGGL((grad_scale_dev_kernel<true, true>), grid, block, 0, as_stream(stream), g, n, record_dev); break;
    }
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}
