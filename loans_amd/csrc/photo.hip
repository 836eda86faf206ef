// Photometric augmentation of a batch that is already resident in HBM (colour jitter, lighting noise, random erasing of
// train_imagenet.py; include/loans_hip.h, loans_photo_*).  x: [B][3][H][W] fp32 in [0, 1]; image n has ONE job (loans_photo_job),
// drawn on the host.  A pixel's three channels are worked on together:
//   grey(r, g, b) = fmaf(0.299f, r, fmaf(0.587f, g, 0.114f * b))
//   brightness    x = clamp01(b * x)
//   saturation    x = clamp01(fmaf(s, x, oms * grey(pixel)))
//   contrast      x = clamp01(fmaf(c, x, cm)),  cm = omc * m,  m = the image's mean grey AS IT STANDS WHEN CONTRAST IS REACHED:
//                 the greys of the pixels after the operations that precede contrast in this image's order, summed in fp64 in
//                 a fixed order, divided by H W in fp64, rounded once to fp32
// in the order the job's code names (a permutation of the three).  A factor that is exactly 1 skips its operation: no clamp, the
// values are a bit copy.  Then, if any addend is non-zero, x = x + add[channel] (no clamp: the lighting noise); last, every pixel
// inside the erase box [y0, y1) x [x0, x1) becomes fill[channel], a bit copy.  An image with all factors 1, a zero addend and an
// empty box leaves bit for bit.  Every multiply-add is an explicit fmaf, so what the compiler would contract is not left to it:
// two launches and two builds give the same bits.  Hue is not built.
//
// Two entries.  photo_grey_kernel runs for the images whose c != 1 (the blocks of the others leave at once): it recomputes the
// operations that precede contrast through photo_ops -- the function the apply pass uses, so the mean is of exactly the values the
// apply pass feeds to contrast --, reduces per wave with shuffles and per block through LDS and writes ONE fp64 partial per (image,
// block) into the caller's workspace; no atomics.  photo_apply_kernel is streaming: every lane owns the same pixels in all three
// planes (three 16-byte loads, three 16-byte stores where W % 4 == 0 and the pointers are 16-byte aligned, else one pixel), so it
// is safe IN PLACE (out == x); the job is uniform over a block and loaded once per image, the order code selects the path without
// lane divergence; the erase box is handled per 16-byte unit (all inside: nothing is read; none inside; mixed).  The partials of an
// image are folded in ascending block order -- one chain of fp64 additions -- by photo_fold_kernel, a small launch of one wave per
// image behind the grey pass (as arena.h folds), which leaves one fp32 mean per image behind the partials; an apply block reads
// that one float.  The other form -- every apply block folding its image's partials in its prologue, one launch fewer -- was timed
// against it and lost: at 256 x 3 x 224 x 224 (49 partials per image) the apply pass took 71.7 us with the fold in its prologue and
// 49.5 us behind the fold launch, which adds 4 us to the grey entry (profiles/imagenet_photo.txt); it is kept under
// LOANS_EXPERIMENT for tools/photo_bench.py.  Grid of the apply pass: the memory-bound idiom of mix.hip, at most 256 CUs x 8 blocks, x over the units of
// an image, y striding over the images.
// Bound: HBM -- in place, one read of the batch for the grey pass plus one read and one write for the apply pass, 3 x B x 3 x H x W
// x 4 bytes (462 MB at 256 x 3 x 224 x 224: 57.8 us at 8 TB/s).  Measured there (profiles/imagenet_photo.txt, tools/photo_bench.py):
// 32.7 us for the grey pass with its fold, 49.5 us for the apply pass (6.23 TB/s), 82.0 us together: 70 % of the bound.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 256 * 8;
constexpr int GREY_PIXELS = 1024;           // pixels per grey-pass block and trip of the 16-byte form: one partial per that many

enum { OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2 };
// order code -> the three operations, two bits each, first operation lowest:
//   0 BCS   1 BSC   2 CBS   3 CSB   4 SBC   5 SCB      (B = 0, C = 1, S = 2: the permutations of (0, 1, 2) in lexicographic order)
__host__ __device__ __forceinline__ unsigned order_ops(int code) {
    constexpr uint64_t table = (uint64_t)(0 | 1 << 2 | 2 << 4) | (uint64_t)(0 | 2 << 2 | 1 << 4) << 6 | (uint64_t)(1 | 0 << 2 | 2 << 4) << 12 |
                               (uint64_t)(1 | 2 << 2 | 0 << 4) << 18 | (uint64_t)(2 | 0 << 2 | 1 << 4) << 24 | (uint64_t)(2 | 1 << 2 | 0 << 4) << 30;
    return (unsigned)(table >> (6 * code)) & 63u;
}

struct Px { float r, g, b; };

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float grey(const Px& p) { return fmaf(0.299f, p.r, fmaf(0.587f, p.g, 0.114f * p.b)); }

// operations [first, last) of the job's order on one pixel; cm is read by contrast alone.  Everything but the pixel is uniform
// over the block.
__device__ __forceinline__ void photo_ops(Px& p, const loans_photo_job& j, unsigned ops, int first, int last, float cm) {
    for (int k = first; k < last; ++k) {
        const unsigned op = (ops >> (2 * k)) & 3u;
        if (op == OP_BRIGHTNESS) {
            if (j.b != 1.f) { p.r = clamp01(j.b * p.r); p.g = clamp01(j.b * p.g); p.b = clamp01(j.b * p.b); }
        } else if (op == OP_SATURATION) {
            if (j.s != 1.f) {
                const float t = j.oms * grey(p);
                p.r = clamp01(fmaf(j.s, p.r, t)); p.g = clamp01(fmaf(j.s, p.g, t)); p.b = clamp01(fmaf(j.s, p.b, t));
            }
        } else {
            if (j.c != 1.f) { p.r = clamp01(fmaf(j.c, p.r, cm)); p.g = clamp01(fmaf(j.c, p.g, cm)); p.b = clamp01(fmaf(j.c, p.b, cm)); }
        }
    }
}

__device__ __forceinline__ int contrast_position(unsigned ops) {
    return (ops & 3u) == OP_CONTRAST ? 0 : (((ops >> 2) & 3u) == OP_CONTRAST ? 1 : 2);
}

// VEC: W % 4 == 0 and 16-byte aligned pointers -- a unit is four pixels of one image row (in each plane), else one pixel.
// units = H * (W / V) per image, under 2^30; element offsets are 64-bit.  gridDim.x == parts: block k of image n writes ws[n * parts + k].
// Order of the additions, fixed: a thread's units ascending (pixel e ascending inside a unit), the xor butterfly inside the wave,
// waves 0..3 through LDS.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void photo_grey_kernel(const float* __restrict__ x, int B, int H, int W, int units,
                                                             const loans_photo_job* __restrict__ jobs, double* __restrict__ ws, int parts) {
    constexpr int V = VEC ? 4 : 1;
    __shared__ double sh[THREADS / 64];
    const int wq = W / V;
    const int64_t plane = (int64_t)H * W;
    for (int n = blockIdx.y; n < B; n += gridDim.y) {
        const loans_photo_job j = jobs[n];
        if (j.c == 1.f) continue;                               // uniform over the block
        const unsigned ops = order_ops(j.order);
        const int npre = contrast_position(ops);
        const float* img = x + (int64_t)n * 3 * plane;
        double acc = 0.0;
        for (int r = blockIdx.x * THREADS + threadIdx.x; r < units; r += gridDim.x * THREADS) {
            const int y = r / wq;
            const int64_t at = (int64_t)y * W + (int64_t)(r - y * wq) * V;
            if (VEC) {
                const f32x4 cr = *reinterpret_cast<const f32x4*>(img + at);
                const f32x4 cg = *reinterpret_cast<const f32x4*>(img + plane + at);
                const f32x4 cb = *reinterpret_cast<const f32x4*>(img + 2 * plane + at);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    Px p{cr[e], cg[e], cb[e]};
                    photo_ops(p, j, ops, 0, npre, 0.f);
                    acc += (double)grey(p);
                }
            } else {
                Px p{img[at], img[plane + at], img[2 * plane + at]};
                photo_ops(p, j, ops, 0, npre, 0.f);
                acc += (double)grey(p);
            }
        }
        acc = wave_sum_d(acc);
        __syncthreads();            // the previous image's sh has been read
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) ws[(int64_t)n * parts + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    }
}

// the partials of image n in ascending block order, the mean in fp64, rounded once: the value every reader of the mean uses
__device__ __forceinline__ float folded_mean(const double* __restrict__ part, int parts, double pixels) {
    double sum = 0.0;
    for (int k = 0; k < parts; ++k) sum += part[k];
    return (float)(sum / pixels);
}

// one wave per image; every lane carries the same chain (broadcast loads), lane 0 stores
__global__ __launch_bounds__(64) void photo_fold_kernel(const loans_photo_job* __restrict__ jobs, const double* __restrict__ ws, int parts,
                                                        double pixels, float* __restrict__ means) {
    const int n = blockIdx.x;
    if (jobs[n].c == 1.f) return;
    const float m = folded_mean(ws + (int64_t)n * parts, parts, pixels);
    if (threadIdx.x == 0) means[n] = m;
}

// PROLOGUE (LOANS_EXPERIMENT builds alone): no fold launch has run, every block folds its image's partials itself
template <bool VEC, bool PROLOGUE>
__global__ __launch_bounds__(THREADS) void photo_apply_kernel(const float* x, float* out, int B, int H, int W, int units,
                                                              const loans_photo_job* __restrict__ jobs, const float* __restrict__ means,
                                                              const double* __restrict__ ws, int parts) {
    constexpr int V = VEC ? 4 : 1;
    const int wq = W / V;
    const int64_t plane = (int64_t)H * W;
    for (int n = blockIdx.y; n < B; n += gridDim.y) {
        const loans_photo_job j = jobs[n];                      // uniform: one load per block and image
        const bool jitter = j.b != 1.f || j.c != 1.f || j.s != 1.f;
        const bool lit = j.add[0] != 0.f || j.add[1] != 0.f || j.add[2] != 0.f;
        const bool boxed = j.y1 > j.y0 && j.x1 > j.x0;
        if (!jitter && !lit && !boxed && out == x) continue;    // the identity, in place: nothing moves
        const unsigned ops = order_ops(j.order);
        float cm = 0.f;
        if (j.c != 1.f) cm = j.omc * (PROLOGUE ? folded_mean(ws + (int64_t)n * parts, parts, (double)plane) : means[n]);
        const float* src = x + (int64_t)n * 3 * plane;
        float* dst = out + (int64_t)n * 3 * plane;
        for (int r = blockIdx.x * THREADS + threadIdx.x; r < units; r += gridDim.x * THREADS) {
            const int y = r / wq;
            const int xa = (r - y * wq) * V;                    // columns [xa, xa + V) of image row y
            const int64_t at = (int64_t)y * W + xa;
            const bool yin = boxed && y >= j.y0 && y < j.y1;
            const bool in_all = yin && xa >= j.x0 && xa + V <= j.x1;
            const bool in_any = yin && xa < j.x1 && xa + V > j.x0;
            if (VEC) {
                f32x4 cr, cg, cb;
                if (in_all) {
                    cr = f32x4{j.fill[0], j.fill[0], j.fill[0], j.fill[0]};
                    cg = f32x4{j.fill[1], j.fill[1], j.fill[1], j.fill[1]};
                    cb = f32x4{j.fill[2], j.fill[2], j.fill[2], j.fill[2]};
                } else {
                    cr = *reinterpret_cast<const f32x4*>(src + at);
                    cg = *reinterpret_cast<const f32x4*>(src + plane + at);
                    cb = *reinterpret_cast<const f32x4*>(src + 2 * plane + at);
                    if (jitter || lit || in_any) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            Px p{cr[e], cg[e], cb[e]};
                            if (jitter) photo_ops(p, j, ops, 0, 3, cm);
                            if (lit) { p.r = p.r + j.add[0]; p.g = p.g + j.add[1]; p.b = p.b + j.add[2]; }
                            if (in_any && xa + e >= j.x0 && xa + e < j.x1) { p.r = j.fill[0]; p.g = j.fill[1]; p.b = j.fill[2]; }
                            cr[e] = p.r; cg[e] = p.g; cb[e] = p.b;
                        }
                    }
                }
                *reinterpret_cast<f32x4*>(dst + at) = cr;
                *reinterpret_cast<f32x4*>(dst + plane + at) = cg;
                *reinterpret_cast<f32x4*>(dst + 2 * plane + at) = cb;
            } else {
                Px p;
                if (in_all) {
                    p = Px{j.fill[0], j.fill[1], j.fill[2]};
                } else {
                    p = Px{src[at], src[plane + at], src[2 * plane + at]};
                    if (jitter) photo_ops(p, j, ops, 0, 3, cm);
                    if (lit) { p.r = p.r + j.add[0]; p.g = p.g + j.add[1]; p.b = p.b + j.add[2]; }
                }
                dst[at] = p.r; dst[plane + at] = p.g; dst[2 * plane + at] = p.b;
            }
        }
    }
}

// partials per image: one per GREY_PIXELS pixels, MAX_BLOCKS at most -- of the sizes alone, whichever form the launch takes
int photo_parts(int64_t pixels) { return grid_for(pixels, GREY_PIXELS, MAX_BLOCKS); }

int grid_y(int B, int gx) {
    const int room = MAX_BLOCKS / gx > 0 ? MAX_BLOCKS / gx : 1;
    return B < room ? B : room;
}

// sizes: LOANS_EINVAL / LOANS_ERANGE / LOANS_OK
int photo_check_sizes(int32_t B, int32_t C, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0 || C != 3) return LOANS_EINVAL;
    if ((int64_t)C * H * W >= ((int64_t)1 << 30)) return LOANS_ERANGE;         // an image is indexed in 32 bits, the batch in 64
    return LOANS_OK;
}

// the host copy of the table: finite numbers, a known order, a box inside the frame; *contrast = whether any image needs its mean
int photo_check_jobs(const loans_photo_job* jobs, int32_t B, int32_t H, int32_t W, bool* contrast) {
    *contrast = false;
    for (int n = 0; n < B; ++n) {
        const loans_photo_job& j = jobs[n];
        const float f[11] = {j.b, j.c, j.s, j.omc, j.oms, j.add[0], j.add[1], j.add[2], j.fill[0], j.fill[1], j.fill[2]};
        for (float v : f)
            if (!__builtin_isfinite(v)) return LOANS_EINVAL;
        if (j.order < 0 || j.order > 5) return LOANS_EINVAL;
        if (!(0 <= j.y0 && j.y0 <= j.y1 && j.y1 <= H && 0 <= j.x0 && j.x0 <= j.x1 && j.x1 <= W)) return LOANS_EINVAL;
        if (j.c != 1.f) *contrast = true;
    }
    return LOANS_OK;
}

}  // namespace

// the workspace: B x parts fp64 partials, then B fp32 means (padded to a multiple of 8 bytes)
extern "C" int64_t loans_photo_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return -1;
    return (int64_t)B * photo_parts((int64_t)H * W) * (int64_t)sizeof(double) + (((int64_t)B * (int64_t)sizeof(float) + 7) & ~(int64_t)7);
}

extern "C" int loans_photo_grey_means_f32(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, const loans_photo_job* jobs_dev,
                                          const loans_photo_job* jobs_host, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!x || !jobs_dev || !jobs_host || !workspace) return LOANS_EINVAL;
    if (((uintptr_t)x & 3) || (((uintptr_t)jobs_dev | (uintptr_t)jobs_host) & 3) || ((uintptr_t)workspace & 7)) return LOANS_EINVAL;
    const int rc = photo_check_sizes(B, C, H, W);
    if (rc != LOANS_OK) return rc;
    if (workspace_bytes < loans_photo_workspace_bytes(B, H, W)) return LOANS_EINVAL;
    bool contrast = false;
    if (photo_check_jobs(jobs_host, B, H, W, &contrast) != LOANS_OK) return LOANS_EINVAL;
    if (!contrast) return LOANS_OK;                             // no image needs a mean: no launch
    const int64_t pixels = (int64_t)H * W;
    const int parts = photo_parts(pixels);
    const bool vec = W % 4 == 0 && ((uintptr_t)x & 15) == 0;
    const int units = (int)(vec ? pixels / 4 : pixels);
    const dim3 grid(parts, grid_y(B, parts));
    double* ws = static_cast<double*>(workspace);
    if (vec)
        hipLaunchKernelGGL(photo_grey_kernel<true>, grid, dim3(THREADS), 0, as_stream(stream), x, B, H, W, units, jobs_dev, ws, parts);
    else
        hipLaunchKernelGGL(photo_grey_kernel<false>, grid, dim3(THREADS), 0, as_stream(stream), x, B, H, W, units, jobs_dev, ws, parts);
    LOANS_LAUNCH_CHECK();
    float* means = reinterpret_cast<float*>(ws + (int64_t)B * parts);
    hipLaunchKernelGGL(photo_fold_kernel, dim3(B), dim3(64), 0, as_stream(stream), jobs_dev, ws, parts, (double)pixels, means);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_photo_apply_f32(const float* x, float* out, int32_t B, int32_t C, int32_t H, int32_t W,
                                     const loans_photo_job* jobs_dev, const loans_photo_job* jobs_host, const void* workspace,
                                     int64_t workspace_bytes, void* stream) {
    if (!x || !out || !jobs_dev || !jobs_host) return LOANS_EINVAL;
    if ((((uintptr_t)x | (uintptr_t)out) & 3) || (((uintptr_t)jobs_dev | (uintptr_t)jobs_host) & 3) || ((uintptr_t)workspace & 7))
        return LOANS_EINVAL;
    const int rc = photo_check_sizes(B, C, H, W);
    if (rc != LOANS_OK) return rc;
    bool contrast = false;
    if (photo_check_jobs(jobs_host, B, H, W, &contrast) != LOANS_OK) return LOANS_EINVAL;
    if (contrast && (!workspace || workspace_bytes < loans_photo_workspace_bytes(B, H, W))) return LOANS_EINVAL;
    const int64_t pixels = (int64_t)H * W;
    const bool vec = W % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
    const int units = (int)(vec ? pixels / 4 : pixels);
    const int gx = grid_for(units, THREADS, MAX_BLOCKS);
    const dim3 grid(gx, grid_y(B, gx));
    const double* ws = static_cast<const double*>(workspace);
    const int parts = photo_parts(pixels);
    const float* means = ws ? reinterpret_cast<const float*>(ws + (int64_t)B * parts) : nullptr;       // read for c != 1 alone
    if (vec)
        hipLaunchKernelGGL((photo_apply_kernel<true, false>), grid, dim3(THREADS), 0, as_stream(stream), x, out, B, H, W, units, jobs_dev, means, ws, parts);
    else
        hipLaunchKernelGGL((photo_apply_kernel<false, false>), grid, dim3(THREADS), 0, as_stream(stream), x, out, B, H, W, units, jobs_dev, means, ws, parts);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

#ifdef LOANS_EXPERIMENT
// The other form of the fold, kept for tools/photo_bench.py to time: the apply pass behind the partials alone, every block folding
// its image's partials in its prologue.  No checks: the tool calls it behind loans_photo_grey_means_f32 with the arguments that
// entry accepted.
extern "C" int loans_photo_exp_apply_prologue_f32(const float* x, float* out, int32_t B, int32_t H, int32_t W, const loans_photo_job* jobs_dev,
                                                  const void* workspace, void* stream) {
    if (!x || !out || !jobs_dev || !workspace || B <= 0 || H <= 0 || W <= 0) return LOANS_EINVAL;
    const int64_t pixels = (int64_t)H * W;
    const bool vec = W % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
    const int units = (int)(vec ? pixels / 4 : pixels);
    const int gx = grid_for(units, THREADS, MAX_BLOCKS);
    const dim3 grid(gx, grid_y(B, gx));
    const double* ws = static_cast<const double*>(workspace);
    const int parts = photo_parts(pixels);
    if (vec)
        hipLaunchKernelGGL((photo_apply_kernel<true, true>), grid, dim3(THREADS), 0, as_stream(stream), x, out, B, H, W, units, jobs_dev, nullptr, ws, parts);
    else
        hipLaunchKernelGGL((photo_apply_kernel<false, true>), grid, dim3(THREADS), 0, as_stream(stream), x, out, B, H, W, units, jobs_dev, nullptr, ws, parts);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}
#endif
