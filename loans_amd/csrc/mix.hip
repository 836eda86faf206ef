// mixup / CutMix of a batch that is already resident in HBM with a shifted copy of itself (the batch-mixing regularisers of
// train_imagenet.py; include/loans_hip.h, loans_batch_mix_f32).  Row b's partner is row p = (b - shift) mod B; per element
//   inside the box [y0, y1) x [x0, x1)     out = x[p]                         a bit copy
//   outside, oml == 0 (uniform)            out = x[b]                         a bit copy: the partner is not read
//   outside, otherwise                     out = fma(lam, x[b], oml * x[p])   one rounding of the product, one of the fma
// (the multiply-add is written as an explicit fmaf, so what the compiler would contract is not left to it: two launches and
// two builds give the same bits).  mixup is an empty box, CutMix a box with (1, 0), "no mixing" an empty box with (1, 0).
// A streaming kernel: no LDS, no atomics, every output element owned by one lane.  Bound: HBM -- three tensor-sized streams
// for mixup (two reads, one write), two for CutMix and for a copy (a 16-byte unit whose pixels all come from one side reads
// that side alone).  The grid is the memory-bound idiom: at most 256 CUs x 8 blocks, x walks the units of a row of the batch,
// y strides over the rows.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 256 * 8;

struct MixBox { int y0, x0, y1, x1; };

// VEC: W % 4 == 0 and both pointers 16-byte aligned -- a unit is four pixels of one image row, else one pixel.
// per_row: units of one row of the batch (C * H * W / (VEC ? 4 : 1)), under 2^30; element offsets are 64-bit.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void batch_mix_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int H, int W,
                                                            int per_row, int shift, float lam, float oml, MixBox box) {
    constexpr int V = VEC ? 4 : 1;
    const bool boxed = box.y1 > box.y0 && box.x1 > box.x0;      // uniform over the launch, like oml == 0 below
    const bool blend = oml != 0.f;
    const int wq = W / V;                                       // units per image row
    const int64_t row_elems = (int64_t)per_row * V;
    for (int r = blockIdx.x * THREADS + threadIdx.x; r < per_row; r += gridDim.x * THREADS) {
        // columns [xa, xa + V) of image row y -- the same for every row of the batch
        bool in_all = false, in_any = false;
        int xa = 0;
        if (boxed) {
            const int line = r / wq;                            // (channel * H + y)
            const int y = line % H;
            xa = (r - line * wq) * V;
            const bool yin = y >= box.y0 && y < box.y1;
            in_all = yin && xa >= box.x0 && xa + V <= box.x1;
            in_any = yin && xa < box.x1 && xa + V > box.x0;
        }
        for (int b = blockIdx.y; b < B; b += gridDim.y) {
            int p = b - shift;
            if (p < 0) p += B;
            const int64_t at = (int64_t)b * row_elems + (int64_t)r * V;
            const int64_t pat = (int64_t)p * row_elems + (int64_t)r * V;
            if (VEC) {
                f32x4 v;
                if (in_all) {
                    v = *reinterpret_cast<const f32x4*>(x + pat);
                } else if (!blend && !in_any) {
                    v = *reinterpret_cast<const f32x4*>(x + at);
                } else {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(x + at);
                    const f32x4 q = *reinterpret_cast<const f32x4*>(x + pat);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool in = in_any && xa + e >= box.x0 && xa + e < box.x1;
                        v[e] = in ? q[e] : (blend ? fmaf(lam, a[e], oml * q[e]) : a[e]);
                    }
                }
                *reinterpret_cast<f32x4*>(out + at) = v;
            } else {
                float v;
                if (in_all) v = x[pat];
                else if (!blend) v = x[at];
                else v = fmaf(lam, x[at], oml * x[pat]);
                out[at] = v;
            }
        }
    }
}

}  // namespace

extern "C" int loans_batch_mix_f32(const float* x, float* out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t shift,
                                   float lam, float oml, int32_t y0, int32_t x0, int32_t y1, int32_t x1, void* stream) {
    if (!x || !out || x == out || B <= 0 || C <= 0 || H <= 0 || W <= 0) return LOANS_EINVAL;
    if (shift < 0 || shift >= B) return LOANS_EINVAL;
    if (!(0 <= y0 && y0 <= y1 && y1 <= H && 0 <= x0 && x0 <= x1 && x1 <= W)) return LOANS_EINVAL;
    if (!__builtin_isfinite(lam) || !__builtin_isfinite(oml)) return LOANS_EINVAL;
    const int64_t row_elems = (int64_t)C * H * W;
    if (row_elems >= ((int64_t)1 << 30)) return LOANS_ERANGE;       // a row of the batch is indexed in 32 bits, the batch in 64
    const bool vec = W % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
    const int per_row = (int)(vec ? row_elems / 4 : row_elems);
    const int gx = grid_for(per_row, THREADS, MAX_BLOCKS);
    const int gy = B < MAX_BLOCKS / gx ? B : (MAX_BLOCKS / gx > 0 ? MAX_BLOCKS / gx : 1);
    const MixBox box{y0, x0, y1, x1};
    if (vec)
        hipLaunchKernelGGL(batch_mix_kernel<true>, dim3(gx, gy), dim3(THREADS), 0, as_stream(stream), x, out, B, H, W, per_row, shift, lam, oml, box);
    else
        hipLaunchKernelGGL(batch_mix_kernel<false>, dim3(gx, gy), dim3(THREADS), 0, as_stream(stream), x, out, B, H, W, per_row, shift, lam, oml, box);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}
