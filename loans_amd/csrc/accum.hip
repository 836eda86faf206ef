// Gradient accumulation over the flat gradient arena (train_imagenet.py --accum-steps K; timm's --grad-accum-steps, DDP's no_sync):
// the gradients of K micro-batches are summed and the optimiser steps once.  For the first n floats of an accumulator `acc` the size
// of the arena and of the gradient arena `g`, one launch per micro-batch:
//   STORE   acc_i = g_i                    the first micro-batch                     g read, acc written:       8 bytes per parameter
//   ADD     acc_i = fl32(acc_i + g_i)      micro-batches 2 .. K - 1                  both read, acc written:   12 bytes per parameter
//   CLOSE   g_i   = fl32(acc_i + g_i)      the last one; acc is left as it is        both read, g written:     12 bytes per parameter
// so the closed gradient is ((g1 + g2) + g3) + .. + gK, one IEEE fp32 addition per element and micro-batch, in that order, and it
// lies where the exchange, the hooks and every optimiser kernel read it.  No scaling (the optimiser's grad_scale carries 1 / K), no
// fp64, no atomic: the bits are torch.add's applied in that order, NaN, inf, signed zeros and subnormals included.  STORE copies
// the bits of g whatever acc held, so an accumulator needs no initialisation.
// Why a buffer and a pass instead of "do not clear the gradients": the fp32 weight gradients do add into the arena, but the bf16
// slab fold, conv1's direct weight-gradient kernel and the BN / bias sums store; this pass leaves every one of them as it is.
#include "arena.h"

namespace {

constexpr int64_t ACCUM_MAX_N = LOANS_GRAD_CLIP_MAX_N;

// One block per unit of ARENA_UNIT floats and trip (u, u + gridDim.x, ..), 64-bit offsets.  A full unit is four float4 of every
// buffer the mode reads per thread, ALL loads issued before the first use (eight in flight for ADD and CLOSE); the last, short unit
// takes float4 while they fit (stride 1024) and single floats for the n & 3 behind them.  Arena offsets are multiples of 8 floats
// and both buffers start on a 16-byte boundary (checked by the entry), so no float4 straddles anything.
// Cache hints, bit 0 of HINT: the loads are non-temporal, bit 1: the store is.  After CLOSE the optimiser's kernel reads g next, as
// after the clip kernel's product; after STORE and ADD acc is not read again for a whole forward and backward and g is cleared by
// the next backward.  tools/accum_bench.py --exp times the four arms of every mode (profiles/imagenet_accum.txt): non-temporal
// loads lose 1.7 - 3.9 us of 30 - 44 in every mode, the store hint is inside the windows' spread (0.1 - 0.2 us); cached / cached is
// compiled for all three -- it has the smallest median for STORE and ADD, and behind CLOSE it is the clip kernel's choice.
template <int MODE, int HINT>
__global__ __launch_bounds__(256) void grad_accum_kernel(float* __restrict__ acc, float* __restrict__ g, int64_t n, int64_t units) {
    constexpr bool NT_LOAD = HINT & 1, NT_STORE = HINT & 2;
    float* const dst = MODE == LOANS_ACCUM_CLOSE ? g : acc;
    auto load = [&](const float* p) { return NT_LOAD ? ldnt4(p) : ld4(p); };
    auto store = [&](float* p, f32x4 v) { if (NT_STORE) stnt4(p, v); else st4(p, v); };
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int64_t off = u * ARENA_UNIT;
        const int64_t left = n - off;
        if (left >= ARENA_UNIT) {
            f32x4 a[4], b[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t at = off + (k * 256 + threadIdx.x) * 4;
                b[k] = load(g + at);
                if (MODE != LOANS_ACCUM_STORE) a[k] = load(acc + at);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t at = off + (k * 256 + threadIdx.x) * 4;
                store(dst + at, MODE == LOANS_ACCUM_STORE ? b[k] : a[k] + b[k]);
            }
        } else if (left > 0) {
            const int m = (int)left, m4 = m & ~3;
            for (int k = threadIdx.x * 4; k < m4; k += 1024) {
                const f32x4 b = load(g + off + k);
                if (MODE == LOANS_ACCUM_STORE) store(dst + off + k, b);
                else store(dst + off + k, load(acc + off + k) + b);
            }
            if ((int)threadIdx.x < (m & 3)) {
                const int64_t at = off + m4 + threadIdx.x;
                dst[at] = MODE == LOANS_ACCUM_STORE ? g[at] : acc[at] + g[at];
            }
        }
    }
}

constexpr int ACCUM_HINT[3] = {0, 0, 0};       // per mode (STORE, ADD, CLOSE): bit 0 non-temporal loads, bit 1 non-temporal store

int accum_hint(int mode) {
#ifdef LOANS_EXPERIMENT
    const char* e = getenv("LOANS_ACCUM_HINT");     // read on every call: the bench interleaves the arms in one process
    if (e && *e) return atoi(e) & 3;
#endif
    return ACCUM_HINT[mode];
}

template <int MODE>
void accum_launch(int hint, dim3 grid, hipStream_t stream, float* acc, float* g, int64_t n, int64_t units) {
    const dim3 block(256);
    switch (hint) {
    case 0: hipLaunchKernelGGL((grad_accum_kernel<MODE, 0>), grid, block, 0, stream, acc, g, n, units); break;
    case 1: hipLaunchKernelGGL((grad_accum_kernel<MODE, 1>), grid, block, 0, stream, acc, g, n, units); break;
    case 2: hipLaunchKernelGGL((grad_accum_kernel<MODE, 2>), grid, block, 0, stream, acc, g, n, units); break;
    default: hipLaunchKernelGGL((grad_accum_kernel<MODE, 3>), grid, block, 0, stream, acc, g, n, units); break;
    }
}

}  // namespace

extern "C" int loans_grad_accum_f32(float* acc, float* g, int64_t n, int32_t mode, void* stream) {
    if (!acc || !g || n <= 0) return LOANS_EINVAL;
    if (((uintptr_t)acc | (uintptr_t)g) & 15) return LOANS_EINVAL;
    if (mode != LOANS_ACCUM_STORE && mode != LOANS_ACCUM_ADD && mode != LOANS_ACCUM_CLOSE) return LOANS_EINVAL;
    if (n > ACCUM_MAX_N) return LOANS_ERANGE;
    const int64_t units = (n + ARENA_UNIT - 1) / ARENA_UNIT;
    const dim3 grid(grid_for(units, 1));
    const int hint = accum_hint(mode);
    switch (mode) {
    case LOANS_ACCUM_STORE: accum_launch<LOANS_ACCUM_STORE>(hint, grid, as_stream(stream), acc, g, n, units); break;
    case LOANS_ACCUM_ADD: accum_launch<LOANS_ACCUM_ADD>(hint, grid, as_stream(stream), acc, g, n, units); break;
    default: accum_launch<LOANS_ACCUM_CLOSE>(hint, grid, as_stream(stream), acc, g, n, units); break;
    }
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}
