// Crop + Pillow BILINEAR resize + `/ 255` + CHW for a batch of frames in ONE launch (the random-resized-crop / centre-crop
// feed of train_imagenet.py; include/loans_hip.h, loans_crop_resize_u8_f32).
//
// The arithmetic is resample.hip's (Pillow's 8-bit resampler, libImaging/Resample.c): per output coordinate a window of the
// input and 22-bit fixed-point coefficients, acc = 2^21 + sum(pixel * k), out = clip8(acc >> 22), horizontal pass first, each
// pass rounds to uint8.  What differs is where the bytes live: the crop is read in place (frame origin + row pitch + box, so
// neither the host nor a copy kernel has to cut it out), and the horizontal pass's output never goes to HBM -- a block owns a
// band of output rows, runs the horizontal pass over the crop rows that band needs into LDS and the vertical pass out of it.
// Bound: HBM (the crop's bytes read + 12 bytes written per output pixel); measured: load latency, 29 % of that bound.
#include "common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr int THREADS = 256;
// Output pixels per block and the LDS of the kernel's two forms, measured (tools/rrc_bench.py, profiles/rrc_feed_ab.txt): the
// kernel is bound by load latency, so what pays is resident waves -- 20 KB lets eight blocks (32 waves, the CU's limit) share a
// CU's 160 KiB, and smaller bands mean more blocks than one round of the machine.  256 crops of 375 x 500 frames -> 224 x 224:
// 32 KB / 4096 pixels 129 us, 16 KB / 4096 105 us, 20 KB / 4096 102 us, 20 KB / 2048 93 us, 20 KB / 1024 100 us.  The 64 KB form
// is for the shapes the small one cannot hold (a vertical window of more than half its rows): long downscales.
constexpr int BAND_PIXELS = 2048;
constexpr int SMALL_LDS_BYTES = 20480;

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

int band_rows(int outH, int outW) {
    int b = BAND_PIXELS / outW;
    if (b < 1) b = 1;
    return b < outH ? b : outH;
}

// one RGB pixel at `a`, column `col` of its frame row, as 0x00BBGGRR | garbage << 24.  Pixels lie at any byte offset, so this is
// an unaligned dword load (gfx9+ global loads take any alignment) of the pixel and ONE neighbouring byte of the same row: the
// byte before it -- except for column 0, whose predecessor may lie in front of the buffer; that one is read byte by byte.
__device__ __forceinline__ uint32_t load_rgb(const uint8_t* a, int col) {
    if (col > 0) {
        uint32_t v;
        __builtin_memcpy(&v, a - 1, 4);
        return v >> 8;
    }
    return (uint32_t)a[0] | ((uint32_t)a[1] << 8) | ((uint32_t)a[2] << 16);
}

constexpr int HROWS = 4;        // crop rows per thread in the horizontal pass: one coefficient load serves four pixels

// VEC: outW % 4 == 0 and dst 16-byte aligned -- the vertical pass takes four pixels (12 LDS bytes, three dwords) per thread
// and stores a float4 per plane.  LDS: bytes of the row image.  SRCS: the jobs' frames lie in several buffers -- job n's
// src_off is relative to srcs[src_index[n]] (`src` is unused); without it the three trailing arguments are unused and the
// instance is the single-source kernel.
template <bool VEC, int LDS, bool SRCS>
__global__ __launch_bounds__(THREADS) void crop_resize_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                              const loans_crop_job* __restrict__ jobs,
                                                              const int32_t* __restrict__ tables, int band, int outH, int outW,
                                                              const uint8_t* const* __restrict__ srcs,
                                                              const int32_t* __restrict__ src_index, int nsrcs) {
    __shared__ __attribute__((aligned(16))) uint8_t rows[LDS];      // [crop rows of this fill][outW][3]
    if (SRCS) {
        // one index per job, read through blockIdx alone: the same for every thread of the block, so a block whose index
        // names no source leaves as a whole, before any barrier and before it has read a job or a pixel
        const int s = src_index[blockIdx.y];
        if (s < 0 || s >= nsrcs) return;
        src = srcs[s];
    }
    const loans_crop_job j = jobs[blockIdx.y];
    const int32_t* hb = tables + j.hb_off;
    const int32_t* hk = tables + j.hk_off;
    const int32_t* vb = tables + j.vb_off;
    const int32_t* vk = tables + j.vk_off;
    const int cap = LDS / (outW * 3);                   // crop rows that fit
    const int64_t plane = (int64_t)outH * outW;
    float* out = dst + (int64_t)blockIdx.y * 3 * plane;
    // pixel (0, 0) of the crop and its column in the frame; with j.flip the crop is the mirror of what lies in memory: its
    // pixel x is pixel w - 1 - x
    const int col0 = j.flip ? j.x0 + j.w - 1 : j.x0;
    const uint8_t* crop = src + j.src_off + (int64_t)j.y0 * j.pitch + (int64_t)col0 * 3;
    const int dir = j.flip ? -1 : 1;

    const int r1 = min((int)(blockIdx.x + 1) * band, outH);
    int yy = blockIdx.x * band;
    // every value that steers this loop comes from blockIdx and the tables: the same for all threads of the block
    while (yy < r1) {
        // the output rows [yy, ye) of this fill: as many as have their crop rows [first, last) inside `cap`
        const int first = vb[2 * yy];
        int last = first, ye = yy;
        while (ye < r1) {
            const int e = vb[2 * ye] + vb[2 * ye + 1];
            if (e - first > cap) break;
            last = e > last ? e : last;
            ++ye;
        }
        if (ye == yy) return;           // one output row needs more rows than fit: the launcher rejects that shape
        const int nrows = last - first;

        // horizontal pass: crop rows [first, last) -> LDS; a thread owns output column xx of HROWS consecutive rows
        const int groups = (nrows + HROWS - 1) / HROWS;
        for (int i = threadIdx.x; i < groups * outW; i += THREADS) {
            const int xx = i % outW, r0 = (i / outW) * HROWS;
            const int xmin = hb[2 * xx], n = hb[2 * xx + 1];
            const int32_t* k = hk + (int64_t)xx * j.hks;
            const int col = col0 + xmin * dir;
            const uint8_t* p[HROWS];
            int acc[HROWS][3];
#pragma unroll
            for (int q = 0; q < HROWS; ++q) {
                // (rows behind the last one repeat it: loaded, never stored)
                const int r = r0 + q < nrows ? r0 + q : nrows - 1;
                p[q] = crop + (int64_t)(first + r) * j.pitch + (int64_t)xmin * dir * 3;
                acc[q][0] = acc[q][1] = acc[q][2] = 1 << (PRECISION_BITS - 1);
            }
            for (int x = 0; x < n; ++x) {
                const int w = k[x];
#pragma unroll
                for (int q = 0; q < HROWS; ++q) {
                    const uint32_t v = load_rgb(p[q] + x * dir * 3, col + x * dir);
                    acc[q][0] += (int)(v & 255) * w;
                    acc[q][1] += (int)((v >> 8) & 255) * w;
                    acc[q][2] += (int)((v >> 16) & 255) * w;
                }
            }
#pragma unroll
            for (int q = 0; q < HROWS; ++q) {
                if (r0 + q < nrows) {
                    uint8_t* o = rows + ((r0 + q) * outW + xx) * 3;
                    o[0] = (uint8_t)clip8(acc[q][0]); o[1] = (uint8_t)clip8(acc[q][1]); o[2] = (uint8_t)clip8(acc[q][2]);
                }
            }
        }
        __syncthreads();

        // vertical pass: LDS -> the three planes of output rows [yy, ye); image / 255 in float32 (IEEE division, as numpy does it)
        if (VEC) {
            const int quads = outW / 4;
            for (int i = threadIdx.x; i < (ye - yy) * quads; i += THREADS) {
                const int x = (i % quads) * 4, o_row = yy + i / quads;
                const int ymin = vb[2 * o_row] - first, n = vb[2 * o_row + 1];
                const int32_t* k = vk + (int64_t)o_row * j.vks;
                const uint32_t* p = reinterpret_cast<const uint32_t*>(rows + (ymin * outW + x) * 3);   // a multiple of 12 bytes
                const int pitch4 = outW * 3 / 4;
                int acc[12];
#pragma unroll
                for (int c = 0; c < 12; ++c) acc[c] = 1 << (PRECISION_BITS - 1);
                for (int y = 0; y < n; ++y) {
                    const int w = k[y];
                    const uint32_t* q = p + y * pitch4;
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const uint32_t v = q[d];
#pragma unroll
                        for (int b = 0; b < 4; ++b) acc[4 * d + b] += (int)((v >> (8 * b)) & 255) * w;
                    }
                }
                // acc[3 * pixel + channel]
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    f32x4 v;
#pragma unroll
                    for (int px = 0; px < 4; ++px) v[px] = (float)clip8(acc[3 * px + c]) / 255.f;
                    *reinterpret_cast<f32x4*>(out + c * plane + (int64_t)o_row * outW + x) = v;
                }
            }
        } else {
            for (int i = threadIdx.x; i < (ye - yy) * outW; i += THREADS) {
                const int x = i % outW, o_row = yy + i / outW;
                const int ymin = vb[2 * o_row] - first, n = vb[2 * o_row + 1];
                const int32_t* k = vk + (int64_t)o_row * j.vks;
                const uint8_t* p = rows + (ymin * outW + x) * 3;
                int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
                for (int y = 0; y < n; ++y) {
                    const int w = k[y];
                    const uint8_t* q = p + y * outW * 3;
                    s0 += (int)q[0] * w;
                    s1 += (int)q[1] * w;
                    s2 += (int)q[2] * w;
                }
                float* o = out + (int64_t)o_row * outW + x;
                o[0] = (float)clip8(s0) / 255.f;
                o[plane] = (float)clip8(s1) / 255.f;
                o[2 * plane] = (float)clip8(s2) / 255.f;
            }
        }
        __syncthreads();                // the next fill overwrites the rows
        yy = ye;
    }
}

}  // namespace

extern "C" int loans_crop_band_rows(int32_t outH, int32_t outW) {
    if (outH <= 0 || outW <= 0) return LOANS_EINVAL;
    return band_rows(outH, outW);
}

extern "C" int loans_crop_resize_u8_f32(const uint8_t* src, float* dst, const loans_crop_job* jobs, int32_t njobs,
                                        const int32_t* tables, int32_t max_vks, int32_t outH, int32_t outW, void* stream) {
    if (!src || !dst || !jobs || !tables || njobs <= 0 || njobs > 65535 || max_vks <= 0 || outH <= 0 || outW <= 0)
        return LOANS_EINVAL;
    if ((int64_t)outW * 3 > LOANS_CROP_LDS_BYTES || max_vks > LOANS_CROP_LDS_BYTES / (outW * 3)) return LOANS_EINVAL;
    if ((int64_t)outH * outW >= ((int64_t)1 << 30)) return LOANS_ERANGE;
    const int band = band_rows(outH, outW);
    const dim3 grid((outH + band - 1) / band, njobs);
    const bool vec = outW % 4 == 0 && ((uintptr_t)dst & 15) == 0;
    const bool small = 2 * max_vks <= SMALL_LDS_BYTES / (outW * 3);     // (at its limit a fill is one output row: every crop row twice)
    auto kern = small ? (vec ? crop_resize_kernel<true, SMALL_LDS_BYTES, false> : crop_resize_kernel<false, SMALL_LDS_BYTES, false>)
                      : (vec ? crop_resize_kernel<true, LOANS_CROP_LDS_BYTES, false> : crop_resize_kernel<false, LOANS_CROP_LDS_BYTES, false>);
    hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, as_stream(stream), src, dst, jobs, tables, band, outH, outW,
                       (const uint8_t* const*)nullptr, (const int32_t*)nullptr, 0);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_crop_resize_srcs_u8_f32(const uint8_t* const* srcs, const int32_t* src_index, int32_t nsrcs, float* dst,
                                             const loans_crop_job* jobs, int32_t njobs, const int32_t* tables, int32_t max_vks,
                                             int32_t outH, int32_t outW, void* stream) {
    if (!srcs || !src_index || nsrcs <= 0) return LOANS_EINVAL;
    // from here on the checks and the choice of the form are those of the single-source entry
    if (!dst || !jobs || !tables || njobs <= 0 || njobs > 65535 || max_vks <= 0 || outH <= 0 || outW <= 0) return LOANS_EINVAL;
    if ((int64_t)outW * 3 > LOANS_CROP_LDS_BYTES || max_vks > LOANS_CROP_LDS_BYTES / (outW * 3)) return LOANS_EINVAL;
    if ((int64_t)outH * outW >= ((int64_t)1 << 30)) return LOANS_ERANGE;
    const int band = band_rows(outH, outW);
    const dim3 grid((outH + band - 1) / band, njobs);
    const bool vec = outW % 4 == 0 && ((uintptr_t)dst & 15) == 0;
    const bool small = 2 * max_vks <= SMALL_LDS_BYTES / (outW * 3);
    auto kern = small ? (vec ? crop_resize_kernel<true, SMALL_LDS_BYTES, true> : crop_resize_kernel<false, SMALL_LDS_BYTES, true>)
                      : (vec ? crop_resize_kernel<true, LOANS_CROP_LDS_BYTES, true> : crop_resize_kernel<false, LOANS_CROP_LDS_BYTES, true>);
    hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, as_stream(stream), (const uint8_t*)nullptr, dst, jobs, tables, band, outH,
                       outW, srcs, src_index, nsrcs);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}
