// Weight gradient of a stride-1 3 x 3 convolution on fp32 tensors with ALL nine taps in one block
// (LOANS_TILE_WGHALO_64 of loans_wgrad_f32; the fp32 counterpart of wgrad_halo_bf16.hip).
//
//     dw[co][t][c] += sum over pixels p of  gy[p][co] * x[p + tap(t)][c]
//
// wgrad_kernel (igemm.hip) computes this as a plain GEMM with (t, c) as columns: every column tile gathers ITS tap's shifted
// copy of x, re-reads gy and redoes the per-pixel row-loader arithmetic for one tap's worth of MFMAs (3.5 - 8.4 non-MFMA
// instructions per MFMA).  Here a 256-thread block owns 64 output x 64 input channels x all nine taps and walks TH x TW pixel
// tiles: per tile it stages the gradient tile [TH * TW px][64] and the zero-filled input HALO tile [(TH + 2) * (TW + 2) px][64]
// ONCE, pixel-major as they lie in memory.  The reduction index of v_mfma_f32_32x32x2_f32 is the pixel: a k-step is two
// horizontally adjacent pixels of one tile row (TW is even), a tap is a constant LDS offset into the halo image.  Pixels
// outside the frame and pixels of ragged tiles hold zeros, so the K loop has no mask and no coordinate arithmetic: per column
// pair and halo row it is 3 input fragments + 1 gradient fragment (ds_read_b32 at lane base + immediate) for up to 9 MFMAs.
//
// LDS rows are 64 floats, unpadded: ds_read_b32 banks are (address / 4) % 32 per 32-lane half, and a half reads 32
// consecutive floats of one pixel -- conflict-free as it lies; the staging writes are contiguous 16-byte units.
// A wave holds one 32 x 32 tile per tap = 144 accumulator registers; two blocks per CU.
// Global loads of tile n + 1 are issued before the MFMAs of tile n and land in registers; the LDS image is single, between
// two barriers (a tile is 28 k-steps x 9 or 49 x 9 MFMAs of 16 passes per wave: the two short write phases hide behind the
// other block of the CU).
// Pixel-tile forms (compile-time, picked by the launcher from the frame): 7 x 14; 7 x 8 where that pads the frame less; and,
// for frames up to 7 x 7, image pairs (wgrad_halo32_pair_kernel below), where a k-step is the same pixel of two images.
#include "common.h"
#include "conv_rows.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// development only: -DLOANS_WGH32_DBG=bits builds the kernel without its atomics (1), with global loads for the first tile
// only (4); 0 in the library
#ifndef LOANS_WGH32_DBG
#define LOANS_WGH32_DBG 0
#endif
constexpr int WGH_DBG = LOANS_WGH32_DBG;

constexpr int BC = 64;                          // channels per block, both operands
constexpr int NT = 256;

struct WgHalo32Args {
    const float* x;
    const float* gy;
    float* dw;
    int B, H, W, Cin, Cout;         // stride 1: input and output share H x W
    int dy0, dx0;                   // taps (dy0 + i, dx0 + j), i, j < 3, row-major = the weight's tap order
    int tiles_y, tiles_x, ntiles;   // pixel tiles per image column / row, in all
    int pairs_co, pairs_c;          // channel tile grid
    int tiles_per_block;
    unsigned x_bytes, gy_bytes;
};

__device__ __forceinline__ u32x4 relu4(u32x4 v) {
    f32x4 f = __builtin_bit_cast(f32x4, v);
    f.x = fmaxf(f.x, 0.f); f.y = fmaxf(f.y, 0.f); f.z = fmaxf(f.z, 0.f); f.w = fmaxf(f.w, 0.f);
    return __builtin_bit_cast(u32x4, f);
}

template <int TH, int TW, bool RELU>
__global__ __launch_bounds__(NT, 2) void wgrad_halo32_kernel(const WgHalo32Args a) {
    static_assert(TW % 2 == 0, "a k-step is two horizontally adjacent pixels");
    constexpr int HH = TH + 2, HW = TW + 2;
    constexpr int YPX = TH * TW, XPX = HH * HW;
    constexpr int UPP = BC / 4;                              // 16-byte units per pixel (16)
    constexpr int PPP = NT / UPP;                            // pixels per loader pass (16)
    constexpr int NGY = (YPX + PPP - 1) / PPP;               // gradient units per thread
    constexpr int NX = (XPX + PPP - 1) / PPP;                // input units per thread
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Ys = reinterpret_cast<float*>(smem);              // [YPX][64]
    float* Xs = Ys + YPX * BC;                               // [XPX][64]

    const int tid = threadIdx.x;
    const int logical = xcd_remap_whole(blockIdx.x, gridDim.x);
    const int npairs = a.pairs_co * a.pairs_c;
    const int split = logical / npairs;
    const int pair = logical - split * npairs;
    const int tco = pair % a.pairs_co, tc = pair / a.pairs_co;
    const int t_begin = split * a.tiles_per_block;
    int t_end = t_begin + a.tiles_per_block;
    if (t_end > a.ntiles) t_end = a.ntiles;
    if (t_begin >= t_end) return;

    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.gy), 0, (int)a.gy_bytes, 0x00020000);

    // this thread's fixed places in the two tiles: channel unit cu of pixels p0 + 16 k (gradient tile) and of halo pixels
    // p0 + 16 k.  Their coordinates are recomputed per tile (divisions by constants, ~100 instructions against a tile's
    // 250 - 440 MFMAs of 16 passes): registers are what this kernel is short of.
    const int cu = tid & (UPP - 1), p0 = tid / UPP;
    const unsigned gch = (unsigned)(tco * BC + cu * 4) * 4u, xch = (unsigned)(tc * BC + cu * 4) * 4u;
    const unsigned gpix = (unsigned)a.Cout * 4u, xpix = (unsigned)a.Cin * 4u;

    u32x4 ry[NGY], rx[NX];
    const int tiles_img = a.tiles_y * a.tiles_x;
    auto load_tile = [&](int t) {
        const int b = t / tiles_img;
        const int rem = t - b * tiles_img;
        const int iy = rem / a.tiles_x;
        const int y0 = iy * TH, x0 = (rem - iy * a.tiles_x) * TW;
        const bool tv = t < t_end;
        const unsigned gbase = (unsigned)((b * a.H + y0) * a.W + x0) * gpix + gch;
        // the halo's first pixel may lie above / left of the image: its (wrapped) offset is only used where the bounds hold
        const unsigned xbase = (unsigned)((b * a.H + y0 + a.dy0) * a.W + x0 + a.dx0) * xpix + xch;
#pragma unroll
        for (int k = 0; k < NGY; ++k) {
            const int p = p0 + k * PPP;
            const int ty = p / TW, tx = p - ty * TW;
            const bool ok = tv & (p < YPX) & (y0 + ty < a.H) & (x0 + tx < a.W);
            const unsigned rel = (unsigned)(ty * a.W + tx) * gpix;
            ry[k] = __builtin_amdgcn_raw_buffer_load_b128(rs_g, (int)((gbase + rel) | ((unsigned)ok - 1u)), 0, 0);
        }
#pragma unroll
        for (int k = 0; k < NX; ++k) {
            const int hp = p0 + k * PPP;
            const int hy = hp / HW, hx = hp - hy * HW;
            const int y = y0 + a.dy0 + hy, x = x0 + a.dx0 + hx;
            const bool ok = tv & (hp < XPX) & ((unsigned)y < (unsigned)a.H) & ((unsigned)x < (unsigned)a.W);
            const unsigned rel = (unsigned)(hy * a.W + hx) * xpix;
            rx[k] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)((xbase + rel) | ((unsigned)ok - 1u)), 0, 0);
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int k = 0; k < NGY; ++k)
            if ((k + 1) * PPP <= YPX || p0 + k * PPP < YPX)
                *reinterpret_cast<u32x4*>(Ys + (p0 + k * PPP) * BC + cu * 4) = ry[k];
#pragma unroll
        for (int k = 0; k < NX; ++k)
            if ((k + 1) * PPP <= XPX || p0 + k * PPP < XPX)
                *reinterpret_cast<u32x4*>(Xs + (p0 + k * PPP) * BC + cu * 4) = RELU ? relu4(rx[k]) : rx[k];
    };

    // fragments of v_mfma_f32_32x32x2_f32: lane (r, h) supplies row / column r of reduction index h = the second pixel of the
    // k-step; the accumulator layout is wgrad_kernel's
    const int wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;                 // 32-channel tiles: gradient (co) x input (c)
    const float* const fragY = Ys + h * BC + wm * 32 + r;
    const float* const fragX = Xs + h * BC + wn * 32 + r;

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

    load_tile(t_begin);
    for (int t = t_begin; t < t_end; ++t) {
        __syncthreads();                    // the previous tile's fragments have been read
        store_tile();
        __syncthreads();
        if constexpr (!(WGH_DBG & 4)) load_tile(t + 1);       // in flight under this tile's MFMAs (nothing is fetched beyond t_end)
#pragma unroll
        for (int q = 0; q < TW / 2; ++q) {
            float ay[3];                    // gradient fragments of output rows rr, rr - 1, rr - 2 (slot = row % 3)
#pragma unroll
            for (int rr = 0; rr < HH; ++rr) {
                // halo row rr = input row y0 + dy0 + rr: it meets output row rr - i under vertical tap i
                if (rr < TH) ay[rr % 3] = fragY[(rr * TW + 2 * q) * BC];
                float bx[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) bx[j] = fragX[(rr * HW + 2 * q + j) * BC];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int orow = rr - i;
                    if (orow >= 0 && orow < TH) {
#pragma unroll
                        for (int j = 0; j < 3; ++j)
                            acc[i * 3 + j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ay[orow % 3], bx[j], acc[i * 3 + j], 0, 0, 0);
                    }
                }
            }
        }
    }

    if constexpr (WGH_DBG & 1) {        // every accumulator stays live
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) sum += acc[t][e];
        if (sum == 123.456f) a.dw[0] = sum;
        return;
    }
    // dw[co][(i, j)][c] += acc: fp32 atomics into the gradient arena (one per element and block)
    const int ktot = 9 * a.Cin;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int col = t * a.Cin + tc * BC + wn * 32 + r;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int co = tco * BC + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            atomic_add_f32(a.dw + (int64_t)co * ktot + col, acc[t][e]);
        }
    }
}

// Frames of at most 7 x 7 pixels (res5): a tile is a PAIR OF IMAGES and a k-step the same pixel of both -- reduction index
// h of the MFMA takes image 2 t + h, whose two LDS images lie a constant offset apart.  Every k-step of a 7 x 7 frame is
// two real pixels (a 7 x 8 tile spends one in eight on its zero column); an odd batch pairs its last image with zeros.  The
// frame fits the tile, so the border of the halo image is zero for every tile: it is cleared once, and per tile only the
// frame's own pixels are loaded and written to their place inside it.
template <bool RELU>
__global__ __launch_bounds__(NT, 2) void wgrad_halo32_pair_kernel(const WgHalo32Args a) {
    constexpr int TH = 7, TW = 7, HH = TH + 2, HW = TW + 2;
    constexpr int YPX = TH * TW, XPX = HH * HW;
    constexpr int UPP = BC / 4, PPP = NT / UPP;
    constexpr int NLD = (2 * YPX + PPP - 1) / PPP;           // units per thread and operand: slot p0 + 16 k of 2 x 49 pixels
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Ys = reinterpret_cast<float*>(smem);              // [2][YPX][64]
    float* Xs = Ys + 2 * YPX * BC;                           // [2][XPX][64]

    const int tid = threadIdx.x;
    const int logical = xcd_remap_whole(blockIdx.x, gridDim.x);
    const int npairs = a.pairs_co * a.pairs_c;
    const int split = logical / npairs;
    const int pair = logical - split * npairs;
    const int tco = pair % a.pairs_co, tc = pair / a.pairs_co;
    const int t_begin = split * a.tiles_per_block;
    int t_end = t_begin + a.tiles_per_block;
    if (t_end > a.ntiles) t_end = a.ntiles;
    if (t_begin >= t_end) return;

    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.gy), 0, (int)a.gy_bytes, 0x00020000);

    const int cu = tid & (UPP - 1), p0 = tid / UPP;
    const unsigned gch = (unsigned)(tco * BC + cu * 4) * 4u, xch = (unsigned)(tc * BC + cu * 4) * 4u;
    const unsigned gpix = (unsigned)a.Cout * 4u, xpix = (unsigned)a.Cin * 4u;

    u32x4 ry[NLD], rx[NLD];
    auto load_tile = [&](int t) {
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int p = p0 + k * PPP;
            const int img = p >= YPX, q = p - img * YPX;
            const int y = q / TW, x = q - y * TW;
            const int b = 2 * t + img;
            const bool ok = (t < t_end) & (p < 2 * YPX) & (b < a.B) & (y < a.H) & (x < a.W);
            const unsigned pixel = (unsigned)((b * a.H + y) * a.W + x);
            ry[k] = __builtin_amdgcn_raw_buffer_load_b128(rs_g, (int)((pixel * gpix + gch) | ((unsigned)ok - 1u)), 0, 0);
            rx[k] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)((pixel * xpix + xch) | ((unsigned)ok - 1u)), 0, 0);
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int p = p0 + k * PPP;
            if ((k + 1) * PPP <= 2 * YPX || p < 2 * YPX) {
                const int img = p >= YPX, q = p - img * YPX;
                const int y = q / TW, x = q - y * TW;
                *reinterpret_cast<u32x4*>(Ys + p * BC + cu * 4) = ry[k];
                // input pixel (y, x) is halo pixel (y - dy0, x - dx0): rows and columns 0 .. 8 for dy0, dx0 in -2 .. 0
                *reinterpret_cast<u32x4*>(Xs + (img * XPX + (y - a.dy0) * HW + (x - a.dx0)) * BC + cu * 4) = RELU ? relu4(rx[k]) : rx[k];
            }
        }
    };

    const int wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const float* const fragY = Ys + h * YPX * BC + wm * 32 + r;
    const float* const fragX = Xs + h * XPX * BC + wn * 32 + r;

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

    load_tile(t_begin);
    {
        const u32x4 z = {0u, 0u, 0u, 0u};
        for (int u = tid; u < 2 * XPX * UPP; u += NT) *reinterpret_cast<u32x4*>(Xs + u * 4) = z;
    }
    for (int t = t_begin; t < t_end; ++t) {
        __syncthreads();                    // the previous tile's fragments have been read (first tile: the halo images are cleared)
        store_tile();
        __syncthreads();
        if constexpr (!(WGH_DBG & 4)) load_tile(t + 1);
#pragma unroll
        for (int q = 0; q < TW; ++q) {
            float ay[3];
#pragma unroll
            for (int rr = 0; rr < HH; ++rr) {
                if (rr < TH) ay[rr % 3] = fragY[(rr * TW + q) * BC];
                float bx[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) bx[j] = fragX[(rr * HW + q + j) * BC];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int orow = rr - i;
                    if (orow >= 0 && orow < TH) {
#pragma unroll
                        for (int j = 0; j < 3; ++j)
                            acc[i * 3 + j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ay[orow % 3], bx[j], acc[i * 3 + j], 0, 0, 0);
                    }
                }
            }
        }
    }

    if constexpr (WGH_DBG & 1) {
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) sum += acc[t][e];
        if (sum == 123.456f) a.dw[0] = sum;
        return;
    }
    const int ktot = 9 * a.Cin;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int col = t * a.Cin + tc * BC + wn * 32 + r;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int co = tco * BC + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            atomic_add_f32(a.dw + (int64_t)co * ktot + col, acc[t][e]);
        }
    }
}

// The pixel-tile form of a frame: image pairs up to 7 x 7 pixels; else 7 x 14 (divides 56, 28 and 14) unless 7 x 8 covers
// the frame with fewer padded pixels.  ops.py mirrors this rule (wghalo_f32_ntiles).
bool pair_tile(int H, int W) { return H <= 7 && W <= 7; }
bool narrow_tile(int H, int W) {
    const int wide = ((H + 6) / 7) * ((W + 13) / 14) * (7 * 14);
    const int narrow = ((H + 6) / 7) * ((W + 7) / 8) * (7 * 8);
    return narrow < wide;
}

// blocks per channel-tile pair the launcher runs for a request (0 = its default)
int plan_splits(WgHalo32Args& a, int splits_req) {
    const int npairs = a.pairs_co * a.pairs_c;
    int splits = splits_req;
    if (splits <= 0) {
        const int cus = loans_device_cus();
        if (cus <= 0) return LOANS_EINVAL;
        splits = (2 * 2 * cus + npairs - 1) / npairs;               // about two rounds of the machine's block slots (two per CU)
        const int max_splits = (a.ntiles + 3) / 4;                  // >= 4 pixel tiles per block: 9 * 32 * 32 partial sums each
        if (splits > max_splits) splits = max_splits;
    }
    if (splits > a.ntiles) splits = a.ntiles;
    if (splits < 1) splits = 1;
    a.tiles_per_block = (a.ntiles + splits - 1) / splits;
    return (a.ntiles + a.tiles_per_block - 1) / a.tiles_per_block;
}

template <int TH, int TW, bool RELU>
int launch(WgHalo32Args& a, int splits_req, hipStream_t st) {
    static loans_device_once lds_limit_set;
    constexpr size_t lds = (size_t)(TH * TW + (TH + 2) * (TW + 2)) * BC * 4;
    static_assert(2 * lds <= 160 * 1024, "two blocks per CU");
    auto kern = wgrad_halo32_kernel<TH, TW, RELU>;
    a.tiles_y = (a.H + TH - 1) / TH; a.tiles_x = (a.W + TW - 1) / TW;
    a.ntiles = a.B * a.tiles_y * a.tiles_x;
    const int splits = plan_splits(a, splits_req);
    if (splits < 0) return splits;
    if (int rc_ = loans_raise_lds_limit(lds_limit_set, reinterpret_cast<const void*>(kern), lds)) return rc_;
    hipLaunchKernelGGL(kern, dim3(a.pairs_co * a.pairs_c * splits), dim3(NT), lds, st, a);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

template <bool RELU>
int launch_pair(WgHalo32Args& a, int splits_req, hipStream_t st) {
    static loans_device_once lds_limit_set;
    constexpr size_t lds = (size_t)2 * (7 * 7 + 9 * 9) * BC * 4;
    static_assert(2 * lds <= 160 * 1024, "two blocks per CU");
    auto kern = wgrad_halo32_pair_kernel<RELU>;
    a.tiles_y = a.tiles_x = 1;
    a.ntiles = (a.B + 1) / 2;
    const int splits = plan_splits(a, splits_req);
    if (splits < 0) return splits;
    if (int rc_ = loans_raise_lds_limit(lds_limit_set, reinterpret_cast<const void*>(kern), lds)) return rc_;
    hipLaunchKernelGGL(kern, dim3(a.pairs_co * a.pairs_c * splits), dim3(NT), lds, st, a);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

}  // namespace

// dw += the gradient by fp32 atomics; the caller (loans_wgrad_f32) has run conv_wgrad_halo_covers
int loans_wgrad_halo32_launch(const float* x, const float* gy, float* dw, const loans_igemm_desc* d, int splits,
                              unsigned x_bytes, unsigned gy_bytes, hipStream_t st) {
    WgHalo32Args a;
    a.x = x; a.gy = gy; a.dw = dw;
    a.B = d->B; a.H = d->inH; a.W = d->inW; a.Cin = d->Cin; a.Cout = d->Cout;
    a.dy0 = d->dy[0]; a.dx0 = d->dx[0];
    a.pairs_co = a.Cout / BC; a.pairs_c = a.Cin / BC;
    a.x_bytes = x_bytes; a.gy_bytes = gy_bytes;
    const bool relu = d->flags & LOANS_F_RELU_IN;
    if (pair_tile(a.H, a.W)) return relu ? launch_pair<true>(a, splits, st) : launch_pair<false>(a, splits, st);
    if (narrow_tile(a.H, a.W))
        return relu ? launch<7, 8, true>(a, splits, st) : launch<7, 8, false>(a, splits, st);
    return relu ? launch<7, 14, true>(a, splits, st) : launch<7, 14, false>(a, splits, st);
}
