// RandAugment / TrivialAugmentWide on a batch that is already resident in HBM (train_imagenet.py --rand-augment / --trivial-augment;
// include/loans_hip.h, loans_ra_*; the arithmetic is stated in loans_amd/common/datasets/rand_augment.py).  x: [B][3][H][W] fp32 in
// [0, 1]; image n has ONE job (loans_ra_job) of 1..4 layers, drawn on the host; a layer is one of fourteen operations:
//   0 Identity
//   1..5 ShearX ShearY TranslateX TranslateY Rotate: nearest-neighbour gather through six 16.16 fixed-point coefficients,
//        xin = (a0 x + a1 y + a2) >> 16, yin = (a3 x + a4 y + a5) >> 16 in 64-bit integers (|a0|, |a1|, |a3|, |a4| <= 2^20, |a2|, |a5| <=
//        2^50, x, y < 2^30: every sum stays below 2^52); a bit copy of src[yin][xin] inside the frame, fill[channel] outside
//   6 Brightness  clamp01(f * x)                         7 Color  clamp01(fmaf(f, x, omf * grey(pixel)))
//   8 Contrast    clamp01(fmaf(f, x, cm)), cm = omf * m, m = the mean grey of the image AS THIS LAYER FINDS IT: fp64 sums in a fixed
//                 order, divided in fp64, rounded once
//   9 Sharpness   interior pixels: acc = the eight neighbours in row-major order added from the left, d = fmaf(5, x, acc) * (1/13),
//                 clamp01(fmaf(f, x, omf * d)); border pixels, and images with H < 3 or W < 3, are bit copies
//  10 Posterize   float(bin(x) & (0xFF << (8 - bits))) / 255,  bin(x) = (int) min(max(fmaf(x, 255, 0.5), 0), 255)
//  11 Solarize    x >= t ? 1 - x : x
//  12 AutoContrast per channel: lo, hi the exact extremes; hi > lo: clamp01((x - lo) * (1 / (hi - lo))), else a bit copy
//  13 Equalize    per channel: h = the 256 counts of bin(x); fewer than two non-zero counts, or step = (sum h - last non-zero h) / 255
//                 == 0: a bit copy; else lut[i] = min(255, (step / 2 + sum_{k < i} h[k]) / step), float(lut[bin(x)]) / 255
// A layer that is the identity for its image (op 0, a zero shear / shift / angle, f == 1, bits == 8, Sharpness on a frame without an
// interior) leaves the image bit for bit.  Every multiply-add is an explicit fmaf; no floating-point atomics: two launches and two
// builds give the same bits.
//
// Per layer at most two steps.  STATISTICS (ra_stats_kernel, ra_fold_kernel) for the images whose layer is Contrast, AutoContrast or
// Equalize -- the blocks of the others leave at once, no launch where there is none --: one record per (image, block) in the
// workspace (the fp64 grey sum; six floats of minima / maxima; 3 x 256 integer counts gathered in LDS), then one block per image
// folds the records in ascending block order and leaves what the apply pass reads: cm; lo, 1 / (hi - lo) and a flag per channel;
// the 3 x 256 table of output floats with a flag per channel.  APPLY (ra_apply_kernel): the job is uniform over a block and selects
// the path without lane divergence; 16-byte units where W % 4 == 0 and the pointers are 16-byte aligned, one pixel otherwise; the
// gathers read single pixels and store units, a wave owning a tile of 8 rows x 8 units so that its sources lie close together.
//
// THE BUFFERS: ping-pong, decided per LAYER for the whole batch on the host, not per image.  The shears, shifts, rotation and
// Sharpness read other pixels than they write; a layer in which any image takes one of them goes from the buffer the batch stands
// in to the other one of {out, a scratch batch in the workspace} -- every image, the untouched ones as copies; a layer of
// pointwise operations alone runs in place and skips its identities.  x is only ever read where out is another tensor: the first
// layer that does anything leaves x, and the destinations are numbered from the end, so that the last one is out.  In place
// (out == x) an odd number of moving layers would end in the scratch batch: one pointwise layer, where the call has one, is taken
// out of place too (the same traffic), else a copy launch follows.  A bit per image would save the copies of the identities in a
// moving layer -- one op in fourteen; with 256 images nearly every layer moves -- at the price of a routing table to validate; the
// feed calls the stage out of place, where no copy launch is ever needed.
// Grid: the memory-bound idiom of photo.hip / mix.hip, at most 256 CUs x 8 blocks, x over the units of an image, y striding over
// the images.  Bound: HBM -- an apply layer reads and writes the batch once (308 MB at 256 x 3 x 224 x 224: 38.5 us at 8 TB/s), a
// statistics step reads it once (19.3 us).  Measured: profiles/imagenet_randaug.txt (tools/randaug_bench.py).
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 256 * 8;
constexpr int STAT_PIXELS = 4096;           // pixels per statistics block and image: one record per that many
constexpr int PART_BYTES = 768 * 4;         // a block's record: 3 x 256 counts (or one double, or six floats, at its start)
constexpr int REC_FLOATS = 784;             // an image's folded record: 768 table entries, three flags, padding to 16 bytes
constexpr int MAX_LAYERS = 4;
constexpr int64_t FIX_ONE = 65536, FIX_HALF = 32768;

enum { RA_IDENTITY = 0, RA_SHEAR_X, RA_SHEAR_Y, RA_TRANSLATE_X, RA_TRANSLATE_Y, RA_ROTATE, RA_BRIGHTNESS, RA_COLOR, RA_CONTRAST,
       RA_SHARPNESS, RA_POSTERIZE, RA_SOLARIZE, RA_AUTOCONTRAST, RA_EQUALIZE, RA_OPS };

struct Px { float r, g, b; };

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float grey(const Px& p) { return fmaf(0.299f, p.r, fmaf(0.587f, p.g, 0.114f * p.b)); }
__device__ __forceinline__ int bin255(float v) { return (int)fminf(fmaxf(fmaf(v, 255.f, 0.5f), 0.f), 255.f); }

// the operation layer l of job j performs on an H x W image: its code, or RA_IDENTITY where it changes nothing
__host__ __device__ __forceinline__ int ra_effective(const loans_ra_job& j, int l, int H, int W) {
    if (l < 0 || l >= j.layers) return RA_IDENTITY;
    const int op = j.op[l];
    if (op >= RA_SHEAR_X && op <= RA_ROTATE) {
        const int64_t* a = j.a[l];
        const bool same = a[0] == FIX_ONE && a[1] == 0 && a[2] == FIX_HALF && a[3] == 0 && a[4] == FIX_ONE && a[5] == FIX_HALF;
        return same ? RA_IDENTITY : op;
    }
    if (op >= RA_BRIGHTNESS && op <= RA_SHARPNESS) {
        if (j.f[l][0] == 1.f) return RA_IDENTITY;
        return (op == RA_SHARPNESS && (H < 3 || W < 3)) ? RA_IDENTITY : op;
    }
    if (op == RA_POSTERIZE) return j.a[l][0] == 8 ? RA_IDENTITY : op;
    return op;
}
__host__ __device__ __forceinline__ bool ra_moves(int op) { return (op >= RA_SHEAR_X && op <= RA_ROTATE) || op == RA_SHARPNESS; }
__host__ __device__ __forceinline__ bool ra_counts(int op) { return op == RA_CONTRAST || op == RA_AUTOCONTRAST || op == RA_EQUALIZE; }

// ---- statistics ------------------------------------------------------------------------------------------------------------------
// VEC: a unit is four pixels of one image row (in each plane), else one pixel.  gridDim.x == parts: block k of image n writes the
// record n * parts + k.  Order of the fp64 additions, fixed: a thread's units ascending (pixel e ascending inside a unit), the xor
// butterfly inside the wave, waves 0..3 through LDS.  Minima, maxima and counts do not depend on an order.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void ra_stats_kernel(const float* __restrict__ x, int B, int H, int W, int units,
                                                           const loans_ra_job* __restrict__ jobs, int layer, char* __restrict__ partials, int parts) {
    constexpr int V = VEC ? 4 : 1;
    __shared__ int hist[768];
    __shared__ double shd[THREADS / 64];
    __shared__ float shm[THREADS / 64][6];
    const int wq = W / V;
    const int64_t plane = (int64_t)H * W;
    for (int n = blockIdx.y; n < B; n += gridDim.y) {
        const int op = ra_effective(jobs[n], layer, H, W);      // uniform over the block
        if (!ra_counts(op)) continue;
        const float* img = x + (int64_t)n * 3 * plane;
        char* rec = partials + ((int64_t)n * parts + blockIdx.x) * PART_BYTES;
        double acc = 0.0;
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        __syncthreads();                                        // the previous image's LDS has been read
        if (op == RA_EQUALIZE) {
            for (int i = threadIdx.x; i < 768; i += THREADS) hist[i] = 0;
            __syncthreads();
        }
        for (int r = blockIdx.x * THREADS + threadIdx.x; r < units; r += gridDim.x * THREADS) {
            const int y = r / wq;
            const int64_t at = (int64_t)y * W + (int64_t)(r - y * wq) * V;
            float c[3][V];
            if (VEC) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(img + k * plane + at);
#pragma unroll
                    for (int e = 0; e < V; ++e) c[k][e] = v[e];
                }
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) c[k][0] = img[k * plane + at];
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                if (op == RA_CONTRAST) {
                    acc += (double)grey(Px{c[0][e], c[1][e], c[2][e]});
                } else if (op == RA_AUTOCONTRAST) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], c[k][e]); hi[k] = fmaxf(hi[k], c[k][e]); }
                } else {
#pragma unroll
                    for (int k = 0; k < 3; ++k) atomicAdd(&hist[k * 256 + bin255(c[k][e])], 1);
                }
            }
        }
        if (op == RA_CONTRAST) {
            acc = wave_sum_d(acc);
            if ((threadIdx.x & 63) == 0) shd[threadIdx.x >> 6] = acc;
            __syncthreads();
            if (threadIdx.x == 0) *reinterpret_cast<double*>(rec) = ((shd[0] + shd[1]) + shd[2]) + shd[3];
        } else if (op == RA_AUTOCONTRAST) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    lo[k] = fminf(lo[k], __shfl_xor(lo[k], o, 64));
                    hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o, 64));
                }
            if ((threadIdx.x & 63) == 0)
                for (int k = 0; k < 3; ++k) { shm[threadIdx.x >> 6][2 * k] = lo[k]; shm[threadIdx.x >> 6][2 * k + 1] = hi[k]; }
            __syncthreads();
            if (threadIdx.x < 6) {
                const int i = threadIdx.x;
                const float a = shm[0][i], b = shm[1][i], c2 = shm[2][i], d = shm[3][i];
                reinterpret_cast<float*>(rec)[i] = (i & 1) ? fmaxf(fmaxf(a, b), fmaxf(c2, d)) : fminf(fminf(a, b), fminf(c2, d));
            }
        } else {
            __syncthreads();
            for (int i = threadIdx.x; i < 768; i += THREADS) reinterpret_cast<int*>(rec)[i] = hist[i];
        }
    }
}

// one block per image: the records in ascending block order -> the image's folded record
__global__ __launch_bounds__(THREADS) void ra_fold_kernel(const loans_ra_job* __restrict__ jobs, int layer, int H, int W,
                                                          const char* __restrict__ partials, int parts, float* __restrict__ folded) {
    __shared__ int h[768];
    const int n = blockIdx.x;
    const loans_ra_job& j = jobs[n];
    const int op = ra_effective(j, layer, H, W);
    if (!ra_counts(op)) return;
    const char* first = partials + (int64_t)n * parts * PART_BYTES;
    float* rec = folded + (int64_t)n * REC_FLOATS;
    if (op == RA_CONTRAST) {
        if (threadIdx.x == 0) {
            double sum = 0.0;
            for (int k = 0; k < parts; ++k) sum += *reinterpret_cast<const double*>(first + (int64_t)k * PART_BYTES);
            const float m = (float)(sum / ((double)H * (double)W));
            rec[0] = j.f[layer][1] * m;
        }
    } else if (op == RA_AUTOCONTRAST) {
        if (threadIdx.x < 3) {
            const int c = threadIdx.x;
            float lo = INFINITY, hi = -INFINITY;
            for (int k = 0; k < parts; ++k) {
                const float* p = reinterpret_cast<const float*>(first + (int64_t)k * PART_BYTES);
                lo = fminf(lo, p[2 * c]);
                hi = fmaxf(hi, p[2 * c + 1]);
            }
            const bool live = hi > lo;
            rec[3 * c] = lo;
            rec[3 * c + 1] = live ? 1.f / (hi - lo) : 0.f;
            rec[3 * c + 2] = live ? 1.f : 0.f;
        }
    } else {
        for (int i = threadIdx.x; i < 768; i += THREADS) {
            int sum = 0;
            for (int k = 0; k < parts; ++k) sum += reinterpret_cast<const int*>(first + (int64_t)k * PART_BYTES)[i];
            h[i] = sum;
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            const int c = threadIdx.x;
            int total = 0, nonzero = 0, last = 0;
            for (int i = 0; i < 256; ++i) {
                const int v = h[c * 256 + i];
                if (v > 0) { ++nonzero; last = v; }
                total += v;
            }
            const int step = (total - last) / 255;
            const bool live = nonzero >= 2 && step > 0;
            rec[768 + c] = live ? 1.f : 0.f;
            if (live) {
                int before = 0;
                for (int i = 0; i < 256; ++i) {
                    const int v = (step / 2 + before) / step;
                    rec[c * 256 + i] = (float)(v < 255 ? v : 255) / 255.f;
                    before += h[c * 256 + i];
                }
            }
        }
    }
}

// ---- apply -----------------------------------------------------------------------------------------------------------------------
// what a pointwise layer holds for one image, uniform over the block
struct Point {
    int op, mask;
    float f, g;                 // f and omf (6, 7, 9); f and cm (8); the threshold (11)
    float lo[3], s[3];
    bool live[3];
};

__device__ __forceinline__ float ra_channel(float v, int c, const Point& q, const float* lut) {
    switch (q.op) {
    case RA_POSTERIZE: return (float)(bin255(v) & q.mask) / 255.f;
    case RA_SOLARIZE: return v >= q.f ? 1.f - v : v;
    case RA_AUTOCONTRAST: return q.live[c] ? clamp01((v - q.lo[c]) * q.s[c]) : v;
    case RA_EQUALIZE: return q.live[c] ? lut[c * 256 + bin255(v)] : v;
    default: return v;
    }
}

__device__ __forceinline__ void ra_point(Px& p, const Point& q, const float* lut) {
    if (q.op == RA_BRIGHTNESS) {
        p.r = clamp01(q.f * p.r); p.g = clamp01(q.f * p.g); p.b = clamp01(q.f * p.b);
    } else if (q.op == RA_COLOR) {
        const float t = q.g * grey(p);
        p.r = clamp01(fmaf(q.f, p.r, t)); p.g = clamp01(fmaf(q.f, p.g, t)); p.b = clamp01(fmaf(q.f, p.b, t));
    } else if (q.op == RA_CONTRAST) {
        p.r = clamp01(fmaf(q.f, p.r, q.g)); p.g = clamp01(fmaf(q.f, p.g, q.g)); p.b = clamp01(fmaf(q.f, p.b, q.g));
    } else {
        p.r = ra_channel(p.r, 0, q, lut); p.g = ra_channel(p.g, 1, q, lut); p.b = ra_channel(p.b, 2, q, lut);
    }
}

// Sharpness of columns [xa, xa + V) of row y of one plane -> o[]; the centre values are c[]
template <int V>
__device__ __forceinline__ void ra_sharp(const float* __restrict__ pl, int y, int xa, int H, int W, float f, float omf, const float* c, float* o) {
    if (y == 0 || y == H - 1) {
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = c[e];
        return;
    }
    float r[3][V + 2];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const float* row = pl + (int64_t)(y - 1 + dy) * W;
        r[dy][0] = xa > 0 ? row[xa - 1] : 0.f;
        r[dy][V + 1] = xa + V < W ? row[xa + V] : 0.f;
        if (V == 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + xa);
#pragma unroll
            for (int e = 0; e < V; ++e) r[dy][e + 1] = v[e];
        } else {
            r[dy][1] = row[xa];
        }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const int xo = xa + e;
        if (xo == 0 || xo == W - 1) { o[e] = c[e]; continue; }
        float acc = r[0][e] + r[0][e + 1];
        acc += r[0][e + 2];
        acc += r[1][e];
        acc += r[1][e + 2];
        acc += r[2][e];
        acc += r[2][e + 1];
        acc += r[2][e + 2];
        const float d = fmaf(5.f, c[e], acc) * (1.f / 13.f);
        o[e] = clamp01(fmaf(f, c[e], omf * d));
    }
}

// layer < 0: no operation at all, a copy of the batch
template <bool VEC>
__global__ __launch_bounds__(THREADS) void ra_apply_kernel(const float* src_batch, float* dst_batch, int B, int H, int W, int units,
                                                           const loans_ra_job* __restrict__ jobs, int layer, const float* __restrict__ folded) {
    constexpr int V = VEC ? 4 : 1;
    __shared__ float lut[768];
    const int wq = W / V;
    const int64_t plane = (int64_t)H * W;
    for (int n = blockIdx.y; n < B; n += gridDim.y) {
        const loans_ra_job& j = jobs[n];                        // uniform: scalar loads of the fields the path reads
        const int op = ra_effective(j, layer, H, W);
        if (op == RA_IDENTITY && src_batch == dst_batch) continue;
        const float* src = src_batch + (int64_t)n * 3 * plane;
        float* dst = dst_batch + (int64_t)n * 3 * plane;
        const float* rec = folded + (int64_t)n * REC_FLOATS;
        const bool gather = op >= RA_SHEAR_X && op <= RA_ROTATE;
        int64_t a[6] = {0, 0, 0, 0, 0, 0};
        float fill[3] = {0.f, 0.f, 0.f};
        Point q{};
        q.op = op;
        if (gather) {
#pragma unroll
            for (int k = 0; k < 6; ++k) a[k] = j.a[layer][k];
#pragma unroll
            for (int k = 0; k < 3; ++k) fill[k] = j.fill[k];
        } else if (op != RA_IDENTITY) {
            q.f = j.f[layer][0];
            q.g = op == RA_CONTRAST ? rec[0] : j.f[layer][1];
            q.mask = op == RA_POSTERIZE ? (0xFF << (8 - (int)j.a[layer][0])) & 0xFF : 0;
            if (op == RA_AUTOCONTRAST) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { q.lo[k] = rec[3 * k]; q.s[k] = rec[3 * k + 1]; q.live[k] = rec[3 * k + 2] != 0.f; }
            } else if (op == RA_EQUALIZE) {
                __syncthreads();                                // the previous image's table has been read
                for (int i = threadIdx.x; i < 768; i += THREADS) lut[i] = rec[i];
#pragma unroll
                for (int k = 0; k < 3; ++k) q.live[k] = rec[768 + k] != 0.f;
                __syncthreads();
            }
        }
        if (gather) {
            // a wave owns a tile of 8 rows x 8 units, not a strip of 64 units: its 64 sources per load lie in a compact patch of the
            // frame (a strip rotated by 30 degrees crosses 128 rows).  The products are formed once per unit, then stepped.
            const int tiles_x = (wq + 7) >> 3, tiles_y = (H + 7) >> 3;
            const int64_t items = (int64_t)tiles_x * tiles_y * 64;
            for (int64_t r = (int64_t)blockIdx.x * THREADS + threadIdx.x; r < items; r += (int64_t)gridDim.x * THREADS) {
                const int64_t tile = r >> 6;
                const int lane = (int)(r & 63);
                const int ty = (int)(tile / tiles_x), tx = (int)(tile - (int64_t)ty * tiles_x);
                const int y = ty * 8 + (lane >> 3), ux = tx * 8 + (lane & 7);
                if (y >= H || ux >= wq) continue;
                const int xa = ux * V;                          // columns [xa, xa + V) of image row y
                const int64_t at = (int64_t)y * W + xa;
                int64_t xs = a[0] * xa + a[1] * y + a[2], ys = a[3] * xa + a[4] * y + a[5];
                float c[3][V];
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const int64_t xin = xs >> 16, yin = ys >> 16;
                    const bool inside = xin >= 0 && xin < W && yin >= 0 && yin < H;
                    const int64_t from = inside ? yin * W + xin : 0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) c[k][e] = inside ? src[k * plane + from] : fill[k];
                    xs += a[0];
                    ys += a[3];
                }
                if (VEC) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) *reinterpret_cast<f32x4*>(dst + k * plane + at) = f32x4{c[k][0], c[k][1 % V], c[k][2 % V], c[k][3 % V]};
                } else {
#pragma unroll
                    for (int k = 0; k < 3; ++k) dst[k * plane + at] = c[k][0];
                }
            }
            continue;
        }
        for (int r = blockIdx.x * THREADS + threadIdx.x; r < units; r += gridDim.x * THREADS) {
            const int y = r / wq;
            const int xa = (r - y * wq) * V;                    // columns [xa, xa + V) of image row y
            const int64_t at = (int64_t)y * W + xa;
            float c[3][V];
            if (VEC) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(src + k * plane + at);
#pragma unroll
                    for (int e = 0; e < V; ++e) c[k][e] = v[e];
                }
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) c[k][0] = src[k * plane + at];
            }
            if (op == RA_SHARPNESS) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    float o[V];
                    ra_sharp<V>(src + k * plane, y, xa, H, W, q.f, q.g, c[k], o);
#pragma unroll
                    for (int e = 0; e < V; ++e) c[k][e] = o[e];
                }
            } else if (op != RA_IDENTITY) {
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    Px p{c[0][e], c[1][e], c[2][e]};
                    ra_point(p, q, lut);
                    c[0][e] = p.r; c[1][e] = p.g; c[2][e] = p.b;
                }
            }
            if (VEC) {
#pragma unroll
                for (int k = 0; k < 3; ++k) *reinterpret_cast<f32x4*>(dst + k * plane + at) = f32x4{c[k][0], c[k][1 % V], c[k][2 % V], c[k][3 % V]};
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) dst[k * plane + at] = c[k][0];
            }
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
int ra_parts(int64_t pixels) { return grid_for(pixels, STAT_PIXELS, MAX_BLOCKS); }

int grid_y(int B, int gx) {
    const int room = MAX_BLOCKS / gx > 0 ? MAX_BLOCKS / gx : 1;
    return B < room ? B : room;
}

int ra_check_sizes(int32_t B, int32_t C, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0 || C != 3) return LOANS_EINVAL;
    if ((int64_t)C * H * W >= ((int64_t)1 << 30)) return LOANS_ERANGE;         // an image is indexed in 32 bits, the batch in 64
    return LOANS_OK;
}

// the host copy of the table: 1..4 layers of known operations with finite parameters, coefficients the 64-bit map cannot
// overflow with, 2..8 bits, a finite fill
int ra_check_jobs(const loans_ra_job* jobs, int32_t B) {
    for (int n = 0; n < B; ++n) {
        const loans_ra_job& j = jobs[n];
        if (j.layers < 1 || j.layers > MAX_LAYERS) return LOANS_EINVAL;
        for (int k = 0; k < 3; ++k)
            if (!__builtin_isfinite(j.fill[k])) return LOANS_EINVAL;
        for (int l = 0; l < j.layers; ++l) {
            const int op = j.op[l];
            if (op < 0 || op >= RA_OPS) return LOANS_EINVAL;
            if (op >= RA_SHEAR_X && op <= RA_ROTATE) {
                const int64_t small = (int64_t)1 << 20, large = (int64_t)1 << 50;
                for (int k = 0; k < 6; ++k) {
                    const int64_t limit = (k == 2 || k == 5) ? large : small;
                    if (j.a[l][k] > limit || j.a[l][k] < -limit) return LOANS_EINVAL;
                }
            } else if (op >= RA_BRIGHTNESS && op <= RA_SHARPNESS) {
                if (!__builtin_isfinite(j.f[l][0]) || !__builtin_isfinite(j.f[l][1])) return LOANS_EINVAL;
            } else if (op == RA_POSTERIZE) {
                if (j.a[l][0] < 2 || j.a[l][0] > 8) return LOANS_EINVAL;
            } else if (op == RA_SOLARIZE) {
                if (!__builtin_isfinite(j.f[l][0])) return LOANS_EINVAL;
            }
        }
    }
    return LOANS_OK;
}

int64_t ra_stat_bytes(int32_t B, int32_t H, int32_t W) {
    return (int64_t)B * ra_parts((int64_t)H * W) * PART_BYTES + (int64_t)B * REC_FLOATS * (int64_t)sizeof(float);
}

struct Workspace {
    char* partials;
    float* folded;
    float* scratch;
};

Workspace ra_carve(void* workspace, int32_t B, int32_t H, int32_t W) {
    char* base = static_cast<char*>(workspace);
    const int64_t parts = ra_parts((int64_t)H * W);
    return Workspace{base, reinterpret_cast<float*>(base + (int64_t)B * parts * PART_BYTES), reinterpret_cast<float*>(base + ra_stat_bytes(B, H, W))};
}

bool ra_layer_has(const loans_ra_job* jobs, int32_t B, int32_t H, int32_t W, int layer, bool (*what)(int)) {
    for (int n = 0; n < B; ++n)
        if (what(ra_effective(jobs[n], layer, H, W))) return true;
    return false;
}
bool ra_acts(int op) { return op != RA_IDENTITY; }

// the statistics step of one layer on the batch `src`; the arguments have been checked
int ra_stats_launch(const float* src, int32_t B, int32_t H, int32_t W, const loans_ra_job* jobs_dev, int layer, const Workspace& ws, hipStream_t st) {
    const int64_t pixels = (int64_t)H * W;
    const int parts = ra_parts(pixels);
    const bool vec = W % 4 == 0 && ((uintptr_t)src & 15) == 0;
    const int units = (int)(vec ? pixels / 4 : pixels);
    const dim3 grid(parts, grid_y(B, parts));
    if (vec)
        hipLaunchKernelGGL(ra_stats_kernel<true>, grid, dim3(THREADS), 0, st, src, B, H, W, units, jobs_dev, layer, ws.partials, parts);
    else
        hipLaunchKernelGGL(ra_stats_kernel<false>, grid, dim3(THREADS), 0, st, src, B, H, W, units, jobs_dev, layer, ws.partials, parts);
    LOANS_LAUNCH_CHECK();
    hipLaunchKernelGGL(ra_fold_kernel, dim3(B), dim3(THREADS), 0, st, jobs_dev, layer, H, W, ws.partials, parts, ws.folded);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

int ra_apply_launch(const float* src, float* dst, int32_t B, int32_t H, int32_t W, const loans_ra_job* jobs_dev, int layer, const Workspace& ws, hipStream_t st) {
    const int64_t pixels = (int64_t)H * W;
    const bool vec = W % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    const int units = (int)(vec ? pixels / 4 : pixels);
    const int gx = grid_for(units, THREADS, MAX_BLOCKS);
    const dim3 grid(gx, grid_y(B, gx));
    if (vec)
        hipLaunchKernelGGL(ra_apply_kernel<true>, grid, dim3(THREADS), 0, st, src, dst, B, H, W, units, jobs_dev, layer, ws.folded);
    else
        hipLaunchKernelGGL(ra_apply_kernel<false>, grid, dim3(THREADS), 0, st, src, dst, B, H, W, units, jobs_dev, layer, ws.folded);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

int ra_check_common(const void* x, int32_t B, int32_t C, int32_t H, int32_t W, const loans_ra_job* jobs_dev, const loans_ra_job* jobs_host,
                    const void* workspace, int64_t workspace_bytes) {
    if (!x || !jobs_dev || !jobs_host || !workspace) return LOANS_EINVAL;
    if (((uintptr_t)x & 3) || (((uintptr_t)jobs_dev | (uintptr_t)jobs_host) & 7) || ((uintptr_t)workspace & 15)) return LOANS_EINVAL;
    const int rc = ra_check_sizes(B, C, H, W);
    if (rc != LOANS_OK) return rc;
    if (workspace_bytes < loans_ra_workspace_bytes(B, H, W)) return LOANS_EINVAL;
    return ra_check_jobs(jobs_host, B);
}

}  // namespace

// the workspace: B x parts block records, B folded records, then a scratch batch of B x 3 x H x W floats
extern "C" int64_t loans_ra_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return -1;
    return ra_stat_bytes(B, H, W) + (int64_t)B * 3 * H * W * (int64_t)sizeof(float);
}

extern "C" int loans_ra_stats_f32(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, const loans_ra_job* jobs_dev,
                                  const loans_ra_job* jobs_host, int32_t layer, void* workspace, int64_t workspace_bytes, void* stream) {
    const int rc = ra_check_common(x, B, C, H, W, jobs_dev, jobs_host, workspace, workspace_bytes);
    if (rc != LOANS_OK) return rc;
    if (layer < 0 || layer >= MAX_LAYERS) return LOANS_EINVAL;
    if (!ra_layer_has(jobs_host, B, H, W, layer, ra_counts)) return LOANS_OK;   // no image needs a statistic: no launch
    return ra_stats_launch(x, B, H, W, jobs_dev, layer, ra_carve(workspace, B, H, W), as_stream(stream));
}

extern "C" int loans_ra_apply_f32(const float* x, float* out, int32_t B, int32_t C, int32_t H, int32_t W, const loans_ra_job* jobs_dev,
                                  const loans_ra_job* jobs_host, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!out || ((uintptr_t)out & 3)) return LOANS_EINVAL;
    const int rc = ra_check_common(x, B, C, H, W, jobs_dev, jobs_host, workspace, workspace_bytes);
    if (rc != LOANS_OK) return rc;
    const Workspace ws = ra_carve(workspace, B, H, W);
    const hipStream_t st = as_stream(stream);
    const bool in_place = x == out;
    // the plan (the header comment, THE BUFFERS): which layers act, which leave the buffer they find the batch in
    bool acts[MAX_LAYERS], away[MAX_LAYERS];
    int moving = 0, first = -1;
    for (int l = 0; l < MAX_LAYERS; ++l) {
        acts[l] = ra_layer_has(jobs_host, B, H, W, l, ra_acts);
        away[l] = ra_layer_has(jobs_host, B, H, W, l, ra_moves);
        moving += away[l];
        if (acts[l] && first < 0) first = l;
    }
    if (first < 0) {                                            // nothing acts: in place nothing moves, else a copy
        return in_place ? LOANS_OK : ra_apply_launch(x, out, B, H, W, jobs_dev, -1, ws, st);
    }
    if (!in_place && !away[first]) { away[first] = true; ++moving; }
    if (in_place && moving % 2 == 1)
        for (int l = 0; l < MAX_LAYERS; ++l)
            if (acts[l] && !away[l]) { away[l] = true; ++moving; break; }
    // destinations numbered from the end: the last moving layer writes out (in place with an odd count: the scratch batch, and
    // a copy follows)
    const float* cur = x;
    int left = moving;
    const int parity = (in_place && moving % 2 == 1) ? 1 : 0;
    for (int l = 0; l < MAX_LAYERS; ++l) {
        if (!acts[l]) continue;
        if (ra_layer_has(jobs_host, B, H, W, l, ra_counts)) {
            const int src_rc = ra_stats_launch(cur, B, H, W, jobs_dev, l, ws, st);
            if (src_rc != LOANS_OK) return src_rc;
        }
        float* dst = const_cast<float*>(cur);
        if (away[l]) {
            --left;
            dst = (left + parity) % 2 == 0 ? out : ws.scratch;
        }
        const int apply_rc = ra_apply_launch(cur, dst, B, H, W, jobs_dev, l, ws, st);
        if (apply_rc != LOANS_OK) return apply_rc;
        cur = dst;
    }
    if (cur != out) return ra_apply_launch(cur, out, B, H, W, jobs_dev, -1, ws, st);
    return LOANS_OK;
}
