// Host-side rules for the convolution launchers (igemm.hip, igemm_bf16.hip, halo_bf16.hip, pw_bf16.hip, wgrad_halo_*.hip,
// stem.hip; not part of the C ABI): what makes a loans_igemm_desc launchable, per entry point.  Plain C++ as well as HIP, no
// HIP calls and no HIP types.  A check sees the descriptor(s), the integer arguments and WHICH pointers are there (CONV_P_*
// bits; `misaligned` = the same bits for address & 15), never an address; it returns LOANS_OK, LOANS_EINVAL or LOANS_ERANGE
// and the entry calls it before it fills an argument struct.  What needs the device (CU counts, LDS limits, the stem's row
// plans, slab planning) stays with the launchers.  tests/conv_desc/test_desc_cpu.py owns these rules.
#pragma once
#include <stdint.h>
#include "loans_hip.h"
#include "conv_rows.h"

enum : unsigned {
    CONV_P_IN = 1, CONV_P_W = 2, CONV_P_OUT = 4, CONV_P_BIAS = 8, CONV_P_STATS = 16, CONV_P_REF = 32, CONV_P_ADDEND = 64,
    CONV_P_W2 = 128, CONV_P_OUT2 = 256, CONV_P_STATS2 = 512,       // the second convolution of a pair
    CONV_P_PARTIAL = 1024, CONV_P_WS = 2048, CONV_P_AFFINE = 4096,
    CONV_P_X = CONV_P_IN, CONV_P_GY = CONV_P_W, CONV_P_DW = CONV_P_OUT      // the weight gradients' names
};

// C/4 float4 groups must tile 256-thread blocks: a divisor of 256, or a multiple of 256 (slabs)
inline bool reduce_channels_ok(int C) {
    if (C < 4 || (C & 3)) return false;
    const int c4 = C / 4;
    return c4 <= 256 ? (256 % c4 == 0) : (c4 % 256 == 0);
}

inline int conv_check_desc(const loans_igemm_desc* d) {
    if (!d) return LOANS_EINVAL;
    if (d->B <= 0 || d->inH <= 0 || d->inW <= 0 || d->Cin <= 0 || (d->Cin & 3)) return LOANS_EINVAL;
    if (d->outH <= 0 || d->outW <= 0 || d->Cout <= 0) return LOANS_EINVAL;
    if (d->gridH <= 0 || d->gridW <= 0 || d->osy <= 0 || d->osx <= 0 || d->isy <= 0 || d->isx <= 0) return LOANS_EINVAL;
    if (d->oy0 < 0 || d->ox0 < 0) return LOANS_EINVAL;
    if ((d->gridH - 1) * d->osy + d->oy0 >= d->outH) return LOANS_EINVAL;
    if ((d->gridW - 1) * d->osx + d->ox0 >= d->outW) return LOANS_EINVAL;
    if (d->ntaps < 1 || d->ntaps > LOANS_MAX_TAPS) return LOANS_EINVAL;
    const int64_t lim = (int64_t)1 << 31;
    if ((int64_t)d->B * d->inH * d->inW * ((d->flags & LOANS_F_DENSE) ? 1 : d->Cin) >= lim) return LOANS_ERANGE;
    if ((int64_t)d->B * d->outH * d->outW * d->Cout >= lim) return LOANS_ERANGE;
    if ((int64_t)d->B * d->gridH * d->gridW >= lim) return LOANS_ERANGE;
    if ((int64_t)d->ntaps * d->Cin * d->Cout >= lim) return LOANS_ERANGE;
    if (d->flags & LOANS_F_DENSE) {
        // no bounds masks in this mode: every K-row of every grid pixel has to lie inside its input row
        for (int t = 0; t < d->ntaps; ++t) {
            if (d->dy[t] < 0 || d->dx[t] < 0) return LOANS_EINVAL;
            if ((d->gridH - 1) * d->isy + d->dy[t] >= d->inH) return LOANS_EINVAL;
            if ((d->gridW - 1) * d->isx + d->dx[t] + d->Cin > d->inW) return LOANS_EINVAL;
        }
    }
    return LOANS_OK;
}

// ---- stem.hip ---------------------------------------------------------------------------------------------------------------
// LOANS_TILE_STEM of loans_igemm_f32
inline int conv_check_stem7(const loans_igemm_desc* d, unsigned misaligned) {
    if (!(d->flags & LOANS_F_DENSE) || (d->flags & ~(LOANS_F_DENSE | LOANS_F_BIAS | LOANS_F_STATS))) return LOANS_EINVAL;
    if (d->ntaps != 7 || d->Cin != 24 || d->Cout != 64 || d->isy != 2 || d->isx != 6) return LOANS_EINVAL;
    // a block's image starts at row 2 oy0 of frame b: 16-byte aligned when row length and row count are even
    if ((d->inW & 1) || (d->inH & 1) || (misaligned & CONV_P_IN) || (misaligned & CONV_P_W)) return LOANS_EINVAL;
    for (int t = 0; t < 7; ++t)
        if (d->dy[t] != t || d->dx[t] != 0) return LOANS_EINVAL;
    if (d->osy != 1 || d->osx != 1 || d->oy0 || d->ox0 || d->outH != d->gridH || d->outW != d->gridW) return LOANS_EINVAL;
    if (2 * (d->gridH - 1) + 7 > d->inH || 6 * (d->gridW - 1) + 24 > d->inW) return LOANS_EINVAL;
    if ((int64_t)d->B * d->inH * d->inW >= ((int64_t)1 << 31) || (int64_t)d->B * d->gridH * d->gridW * 64 >= ((int64_t)1 << 31))
        return LOANS_ERANGE;
    return LOANS_OK;
}

// LOANS_TILE_STEM of loans_igemm_bf16_f32 (out_bf16 = 1: LOANS_F_OUT_BF16 required) and of loans_igemm_bf16s (0: implied, not set)
inline int conv_check_stem7_bf16(const loans_igemm_desc* d, unsigned misaligned, int out_bf16) {
    if (out_bf16 ? !(d->flags & LOANS_F_OUT_BF16) : (d->flags & LOANS_F_OUT_BF16)) return LOANS_EINVAL;
    if (!(d->flags & LOANS_F_DENSE) || (d->flags & ~(LOANS_F_DENSE | LOANS_F_OUT_BF16 | LOANS_F_BIAS | LOANS_F_STATS))) return LOANS_EINVAL;
    if (d->ntaps != 7 || d->Cin != 24 || d->Cout != 64 || d->isy != 2 || d->isx != 6) return LOANS_EINVAL;
    if ((d->inW & 1) || (d->inH & 1) || (misaligned & CONV_P_IN) || (misaligned & CONV_P_W) || (misaligned & CONV_P_OUT))
        return LOANS_EINVAL;
    for (int t = 0; t < 7; ++t)
        if (d->dy[t] != t || d->dx[t] != 0) return LOANS_EINVAL;
    if (d->osy != 1 || d->osx != 1 || d->oy0 || d->ox0 || d->outH != d->gridH || d->outW != d->gridW) return LOANS_EINVAL;
    if (2 * (d->gridH - 1) + 7 > d->inH || 6 * (d->gridW - 1) + 24 > d->inW) return LOANS_EINVAL;
    if ((int64_t)d->B * d->inH * d->inW >= ((int64_t)1 << 31) || (int64_t)d->B * d->gridH * d->gridW * 64 >= ((int64_t)1 << 31))
        return LOANS_ERANGE;
    return LOANS_OK;
}

// LOANS_TILE_STEM of loans_wgrad_f32, up to the kernel's LDS limit (the byte sizes follow it: conv_stem7_wgrad_bytes)
inline int conv_check_stem7_wgrad(const loans_igemm_desc* d, unsigned misaligned) {
    if (d->flags != LOANS_F_DENSE) return LOANS_EINVAL;
    if (d->ntaps != 7 || d->Cin != 24 || d->Cout != 64 || d->isy != 2 || d->isx != 6) return LOANS_EINVAL;
    if ((d->inW & 1) || (d->inH & 1) || (misaligned & CONV_P_X) || (misaligned & CONV_P_GY)) return LOANS_EINVAL;
    for (int t = 0; t < 7; ++t)
        if (d->dy[t] != t || d->dx[t] != 0) return LOANS_EINVAL;
    if (d->osy != 1 || d->osx != 1 || d->oy0 || d->ox0 || d->outH != d->gridH || d->outW != d->gridW) return LOANS_EINVAL;
    if (2 * (d->gridH - 1) + 7 > d->inH || 6 * (d->gridW - 1) + 24 > d->inW) return LOANS_EINVAL;
    if ((int64_t)d->B * d->inH * d->inW >= ((int64_t)1 << 31) || (int64_t)d->B * d->gridH * d->gridW * 64 >= ((int64_t)1 << 31))
        return LOANS_ERANGE;
    return LOANS_OK;
}

inline int conv_stem7_wgrad_bytes(const loans_igemm_desc* d, unsigned* x_bytes, unsigned* gy_bytes) {
    const int64_t xb = (int64_t)d->B * d->inH * d->inW * 4, gb = (int64_t)d->B * d->gridH * d->gridW * 256;
    if (xb >= 0xFFFFFFF0ll || gb >= 0xFFFFFFF0ll) return LOANS_ERANGE;
    *x_bytes = (unsigned)xb; *gy_bytes = (unsigned)gb;
    return LOANS_OK;
}

// LOANS_TILE_STEM of loans_wgrad_bf16s: 1 if the geometry is the stem's (the kernel's own tile limits stay in stem.hip)
inline int conv_stem7_wgrad_bf16_covers(const loans_igemm_desc* d) {
    if (d->flags != LOANS_F_DENSE) return 0;
    if (d->ntaps != 7 || d->Cin != 24 || d->Cout != 64 || d->isy != 2 || d->isx != 6) return 0;
    if ((d->inH & 1) || (d->gridW & 15)) return 0;
    if (d->inW != 6 * (d->gridW + 3)) return 0;                 // rows of whole 12-byte cells, Wo + 3 of them (even frame widths)
    for (int t = 0; t < 7; ++t)
        if (d->dy[t] != t || d->dx[t] != 0) return 0;
    if (d->osy != 1 || d->osx != 1 || d->oy0 || d->ox0 || d->outH != d->gridH || d->outW != d->gridW) return 0;
    if (2 * (d->gridH - 1) + 7 > d->inH) return 0;
    return 1;
}

inline int conv_stem7_wgrad_bf16_bytes(const loans_igemm_desc* d, unsigned* x_bytes, unsigned* gy_bytes) {
    const int64_t xb = (int64_t)d->B * d->inH * d->inW * 2, gb = (int64_t)d->B * d->gridH * d->gridW * 128;
    if (xb >= 0x7FFFFFF0ll || gb >= 0x7FFFFFF0ll) return LOANS_ERANGE;       // bit 31 of an offset marks a piece that is not loaded
    *x_bytes = (unsigned)xb; *gy_bytes = (unsigned)gb;
    return LOANS_OK;
}

// ---- halo_bf16.hip, pw_bf16.hip, wgrad_halo_*.hip ---------------------------------------------------------------------------
// 1 if the descriptor is a geometry the halo kernels cover (conv_check_igemm16 has validated everything else)
inline int conv_halo16_covers(const loans_igemm_desc* d, int tile) {
    if (d->flags & LOANS_F_DENSE) return 0;
    if ((d->flags & LOANS_F_BNSUMS) && tile == LOANS_TILE_WS64) return 0;        // ws8_kernel's epilogue does not take the BN sums
    if (d->isy != 1 || d->isx != 1 || d->osy != 1 || d->osx != 1 || d->oy0 || d->ox0) return 0;
    if (d->gridH != d->outH || d->gridW != d->outW) return 0;
    if (d->Cin % 64 || d->ntaps > 9) return 0;
    if ((tile == LOANS_TILE_HALO_256x64 || tile == LOANS_TILE_HALO_128x64S) && d->Cin != 64) return 0;
    if ((tile == LOANS_TILE_WS64 || tile == LOANS_TILE_WSW64) && (d->Cin != 64 || d->Cout > 64 || d->ntaps != 9 || (d->flags & LOANS_F_RELU_IN))) return 0;
    int nx = 1;
    while (nx < d->ntaps && d->dy[nx] == d->dy[0]) ++nx;
    if (d->ntaps % nx) return 0;
    const int ny = d->ntaps / nx;
    if (nx > 3 || ny > 3) return 0;
    const int sdx = nx > 1 ? d->dx[1] - d->dx[0] : 1, sdy = ny > 1 ? d->dy[nx] - d->dy[0] : 1;
    if ((sdx != 1 && sdx != -1) || (sdy != 1 && sdy != -1)) return 0;
    for (int t = 0; t < d->ntaps; ++t)
        if (d->dy[t] != d->dy[0] + (t / nx) * sdy || d->dx[t] != d->dx[0] + (t % nx) * sdx) return 0;
    return 1;
}

// loans_halo16_launch, up to the tile's own grid
inline int conv_check_halo16(const loans_igemm_desc* d, int tile, unsigned in_bytes, unsigned w_bytes) {
    if (!conv_halo16_covers(d, tile)) return LOANS_EINVAL;
    if (in_bytes >= 0x80000000u || w_bytes >= 0x80000000u) return LOANS_ERANGE;       // offsets >= 2^31 mean "no load" here
    int nx = 1;
    while (nx < d->ntaps && d->dy[nx] == d->dy[0]) ++nx;
    const int ny = d->ntaps / nx;
    if ((tile == LOANS_TILE_WS64 || tile == LOANS_TILE_WSW64) && !(nx == 3 && ny == 3)) return LOANS_EINVAL;
    return LOANS_OK;
}

// what LOANS_TILE_PW covers: a 1 x 1 / 1 forward geometry (grid = input = output pixels), Cin in {64, 128} with Cout a multiple of 64
// up to 512, or Cin = 256 with Cout a multiple of 128 up to 1024; flags STATS or none
inline int conv_pw16_covers(const loans_igemm_desc* d) {
    if (d->ntaps != 1 || d->dy[0] != 0 || d->dx[0] != 0) return 0;
    if (d->isy != 1 || d->isx != 1 || d->osy != 1 || d->osx != 1 || d->oy0 != 0 || d->ox0 != 0) return 0;
    if (d->gridH != d->inH || d->gridW != d->inW || d->gridH != d->outH || d->gridW != d->outW) return 0;
    if (d->Cin == 256) {
        if (d->Cout % 128 != 0 || d->Cout < 128 || d->Cout > 1024) return 0;
    } else {
        if (d->Cin != 64 && d->Cin != 128) return 0;
        if (d->Cout % 64 != 0 || d->Cout < 64 || d->Cout > 512) return 0;
    }
    if (d->flags & ~(LOANS_F_STATS | LOANS_F_AFFINE_IN)) return 0;
    return 1;
}

// loans_pw16_launch; `have`: CONV_P_STATS, CONV_P_AFFINE
inline int conv_check_pw16(const loans_igemm_desc* d, unsigned have) {
    if (!conv_pw16_covers(d)) return LOANS_EINVAL;
    const int64_t M64 = (int64_t)d->B * d->gridH * d->gridW;
    if (M64 <= 0 || M64 > 0x7FFFFFFF - 64) return LOANS_ERANGE;
    if ((d->flags & LOANS_F_STATS) && !(have & CONV_P_STATS)) return LOANS_EINVAL;
    if ((d->flags & LOANS_F_AFFINE_IN) && !(have & CONV_P_AFFINE)) return LOANS_EINVAL;
    return LOANS_OK;
}

// LOANS_TILE_WGHALO_* of loans_wgrad_bf16s covers: the forward geometry of a stride-1 convolution with a 3 x 3 tap grid (row-major,
// any padding), Cin % 64 == 0, Cout % (64 | 128) == 0, not the dense RGB layout
inline int conv_wgrad_halo16_covers(const loans_igemm_desc* d, int tile) {
    if (tile != LOANS_TILE_WGHALO_64 && tile != LOANS_TILE_WGHALO_128) return 0;
    if (d->flags & ~LOANS_F_RELU_IN) return 0;
    if (d->isy != 1 || d->isx != 1 || d->osy != 1 || d->osx != 1 || d->oy0 || d->ox0) return 0;
    if (d->inH != d->outH || d->inW != d->outW || d->gridH != d->outH || d->gridW != d->outW) return 0;
    if ((d->Cin % 64) || (d->Cout % (tile == LOANS_TILE_WGHALO_64 ? 64 : 128))) return 0;
    if (d->ntaps != 9) return 0;
    for (int t = 0; t < 9; ++t)
        if (d->dy[t] != d->dy[0] + t / 3 || d->dx[t] != d->dx[0] + t % 3) return 0;
    if (d->dy[0] < -2 || d->dy[0] > 0 || d->dx[0] < -2 || d->dx[0] > 0) return 0;
    if ((int64_t)d->B * d->inH * d->inW * (d->Cin > d->Cout ? d->Cin : d->Cout) * 2 >= 0xFFFFFFF0ll) return 0;
    return 1;
}

// LOANS_TILE_WGHALO_64 of loans_wgrad_f32 covers: the same with Cout % 64 == 0
inline int conv_wgrad_halo32_covers(const loans_igemm_desc* d) {
    if (d->flags & ~LOANS_F_RELU_IN) return 0;
    if (d->isy != 1 || d->isx != 1 || d->osy != 1 || d->osx != 1 || d->oy0 || d->ox0) return 0;
    if (d->inH != d->outH || d->inW != d->outW || d->gridH != d->outH || d->gridW != d->outW) return 0;
    if ((d->Cin % 64) || (d->Cout % 64)) return 0;
    if (d->ntaps != 9) return 0;
    for (int t = 0; t < 9; ++t)
        if (d->dy[t] != d->dy[0] + t / 3 || d->dx[t] != d->dx[0] + t % 3) return 0;
    if (d->dy[0] < -2 || d->dy[0] > 0 || d->dx[0] < -2 || d->dx[0] > 0) return 0;
    return 1;
}

// ---- igemm.hip --------------------------------------------------------------------------------------------------------------
// loans_igemm_f32 / loans_igemm_bf16_f32 (bf16 = 1), a pair launch (pair: the second convolution has pair_cout channels) or a
// class launch (ncls >= 2: descs[0] is `d`; bit c of w_have = the weights of class c are there)
inline int conv_check_igemm32(const loans_igemm_desc* d, unsigned have, unsigned misaligned, int bf16, bool pair = false,
                              int pair_cout = 0, int ncls = 0, const loans_igemm_desc* descs = nullptr, unsigned w_have = 0) {
    const bool mc = ncls > 0;
    int rc = conv_check_desc(d);
    if (rc) return rc;
    if (!(have & CONV_P_IN) || !(have & CONV_P_W) || !(have & CONV_P_OUT) || (d->Cout & 3)) return LOANS_EINVAL;
    if ((d->flags & LOANS_F_BIAS) && !(have & CONV_P_BIAS)) return LOANS_EINVAL;
    if ((d->flags & LOANS_F_STATS) && !(have & CONV_P_STATS)) return LOANS_EINVAL;
    if ((d->flags & (LOANS_F_MASK | LOANS_F_ADDEND_MASK)) && !(have & CONV_P_REF)) return LOANS_EINVAL;
    if ((d->flags & LOANS_F_ADDEND_MASK) && !(d->flags & LOANS_F_ADDEND)) return LOANS_EINVAL;
    if ((d->flags & LOANS_F_ADDEND) && !(have & CONV_P_ADDEND)) return LOANS_EINVAL;
    if ((d->flags & LOANS_F_OUT_BF16) && (d->flags & (LOANS_F_MASK | LOANS_F_ADDEND | LOANS_F_ADDEND_MASK))) return LOANS_EINVAL;
    if (d->flags & LOANS_F_BNSUMS) {        // a data gradient's epilogue takes the sums of the BN below it: nothing else rides along
        if (!(have & CONV_P_REF) || !(have & CONV_P_BIAS) || !(have & CONV_P_STATS) || pair || mc) return LOANS_EINVAL;
        if (d->flags & (LOANS_F_BIAS | LOANS_F_STATS | LOANS_F_MASK | LOANS_F_ADDEND | LOANS_F_ADDEND_MASK | LOANS_F_DENSE | LOANS_F_OUT_BF16))
            return LOANS_EINVAL;
        if ((d->tile & 0xEF) == LOANS_TILE_FINETAIL) return LOANS_EINVAL;
    }
    const int Ktot = d->ntaps * d->Cin;
    {
        const int64_t ib = (int64_t)d->B * d->inH * d->inW * ((d->flags & LOANS_F_DENSE) ? 1 : d->Cin) * 4;
        const int64_t wb = (int64_t)d->Cout * Ktot * 4;
        const int64_t ob = (int64_t)d->B * d->outH * d->outW * d->Cout * ((d->flags & LOANS_F_OUT_BF16) ? 2 : 4);
        if (ib >= 0xFFFFFFF0ll || wb >= 0xFFFFFFF0ll || ob >= 0xFFFFFFF0ll) return LOANS_ERANGE;   // 32-bit buffer offsets
    }
    if (pair) {
        const int64_t wb2 = (int64_t)pair_cout * Ktot * 4;
        const int64_t ob2 = (int64_t)d->B * d->outH * d->outW * pair_cout * 4;
        if (wb2 >= 0xFFFFFFF0ll || ob2 >= 0xFFFFFFF0ll) return LOANS_ERANGE;
    }
    if (mc) {
        // the classes differ in their grid, their output phase and their taps; image, strides, channels and flags are shared
        if (pair || bf16 || ncls < 2 || ncls > LOANS_MAX_CLASSES) return LOANS_EINVAL;
        if (d->flags & (LOANS_F_DENSE | LOANS_F_STATS | LOANS_F_BIAS)) return LOANS_EINVAL;
        for (int c = 0; c < ncls; ++c) {
            const loans_igemm_desc* e = descs + c;
            if ((rc = conv_check_desc(e))) return rc;
            if (!((w_have >> c) & 1) || e->ntaps > LOANS_MAX_CLS_TAPS) return LOANS_EINVAL;
            if (e->B != d->B || e->inH != d->inH || e->inW != d->inW || e->Cin != d->Cin || e->outH != d->outH ||
                e->outW != d->outW || e->Cout != d->Cout || e->osy != d->osy || e->osx != d->osx || e->isy != d->isy ||
                e->isx != d->isx || e->flags != d->flags)
                return LOANS_EINVAL;
        }
    }
    int tile = d->tile;
    if (mc) {
        const int t = tile & ~LOANS_TILE_DMA;
        if (t != LOANS_TILE_128x128 && t != LOANS_TILE_128x64 && t != LOANS_TILE_64x64 && t != LOANS_TILE_256x64) return LOANS_EINVAL;
    }
    if (pair && ((tile >> 8) || (tile & 0xFF) == LOANS_TILE_SPLIT)) return LOANS_EINVAL;
    int splits = (tile >> 8) & 0xFF;        // LOANS_TILE_SPLITK(s)
    if (splits < 1) splits = 1;
    tile &= 0xFF;
    if (splits > 1 && (bf16 || (d->flags & ~(LOANS_F_DENSE | LOANS_F_RELU_IN)) || tile == LOANS_TILE_SPLIT))
        return LOANS_EINVAL;                // raw partial sums only: the epilogue flags belong to loans_igemm_finalize_f32
    const int dma = (tile & LOANS_TILE_DMA) ? 1 : 0;
    if (dma && bf16) return LOANS_EINVAL;
    tile &= ~LOANS_TILE_DMA;
    if (tile == LOANS_TILE_STEM) {          // the dense RGB stem as a direct convolution (stem.hip)
        if (pair || splits > 1 || dma || mc) return LOANS_EINVAL;
        return bf16 ? conv_check_stem7_bf16(d, misaligned, 1) : conv_check_stem7(d, misaligned);
    }
    if (tile == LOANS_TILE_FINETAIL) {
        if (pair || bf16 || splits > 1) return LOANS_EINVAL;
        if (d->flags & (LOANS_F_MASK | LOANS_F_ADDEND | LOANS_F_ADDEND_MASK | LOANS_F_OUT_BF16)) return LOANS_EINVAL;
        if (d->osy != 1 || d->osx != 1 || d->oy0 || d->ox0 || d->outH != d->gridH || d->outW != d->gridW) return LOANS_EINVAL;
        const int c4 = d->Cout / 4;
        if ((d->Cout & 3) || !(c4 <= 256 ? (256 % c4 == 0) : (c4 % 256 == 0))) return LOANS_EINVAL;   // finalize's thread map
        return LOANS_OK;
    }
    switch (tile) {
        case 0: case LOANS_TILE_SPLIT:
        case LOANS_TILE_128x128: case LOANS_TILE_128x64: case LOANS_TILE_64x64: case LOANS_TILE_256x64: return LOANS_OK;
        default: return LOANS_EINVAL;
    }
}

inline int conv_check_igemm_f32(const loans_igemm_desc* d, unsigned have, unsigned misaligned) { return conv_check_igemm32(d, have, misaligned, 0); }
inline int conv_check_igemm_bf16_f32(const loans_igemm_desc* d, unsigned have, unsigned misaligned) { return conv_check_igemm32(d, have, misaligned, 1); }

inline int conv_check_igemm_pair_f32(const loans_igemm_desc* d, unsigned have, unsigned misaligned, int Cout_b) {
    if (!d || !(have & CONV_P_W2) || !(have & CONV_P_OUT2) || Cout_b <= 0 || (Cout_b & 3)) return LOANS_EINVAL;
    if (d->flags & ~(LOANS_F_STATS | LOANS_F_RELU_IN)) return LOANS_EINVAL;
    if ((d->flags & LOANS_F_STATS) && !(have & CONV_P_STATS2)) return LOANS_EINVAL;
    return conv_check_igemm32(d, have & ~(CONV_P_BIAS | CONV_P_REF | CONV_P_ADDEND), misaligned, 0, true, Cout_b);
}

// have_w: the array of weight pointers is there; bit c of w_have: so is its entry c
inline int conv_check_igemm_classes_f32(const loans_igemm_desc* descs, int n, unsigned have, unsigned misaligned, bool have_w,
                                        unsigned w_have) {
    if (!descs || !have_w || n < 1) return LOANS_EINVAL;
    have = (have & ~(CONV_P_W | CONV_P_BIAS | CONV_P_STATS)) | ((w_have & 1) ? CONV_P_W : 0u);
    if (n == 1) return conv_check_igemm32(descs, have, misaligned, 0);
    return conv_check_igemm32(descs, have, misaligned, 0, false, 0, n, descs, w_have);
}

inline int conv_check_finalize_f32(unsigned have, int flags, int64_t rows, int C) {
    if (!(have & CONV_P_OUT) || rows <= 0 || !reduce_channels_ok(C)) return LOANS_EINVAL;
    if ((flags & LOANS_F_BIAS) && !(have & CONV_P_BIAS)) return LOANS_EINVAL;
    if ((flags & LOANS_F_STATS) && !(have & CONV_P_STATS)) return LOANS_EINVAL;
    if ((flags & (LOANS_F_MASK | LOANS_F_ADDEND_MASK)) && !(have & CONV_P_REF)) return LOANS_EINVAL;
    if ((flags & LOANS_F_ADDEND_MASK) && !(flags & LOANS_F_ADDEND)) return LOANS_EINVAL;
    if ((flags & LOANS_F_ADDEND) && !(have & CONV_P_ADDEND)) return LOANS_EINVAL;
    if (flags & ~(LOANS_F_BIAS | LOANS_F_STATS | LOANS_F_MASK | LOANS_F_ADDEND | LOANS_F_ADDEND_MASK)) return LOANS_EINVAL;
    return LOANS_OK;
}

// loans_wgrad_f32 / loans_wgrad_bf16_f32 (bf16 = 1)
inline int conv_check_wgrad32(const loans_igemm_desc* d, unsigned have, unsigned misaligned, int bf16) {
    int rc = conv_check_desc(d);
    if (rc) return rc;
    if (!(have & CONV_P_X) || !(have & CONV_P_GY) || !(have & CONV_P_DW) || (d->Cout & 3)) return LOANS_EINVAL;
    const int Ktot = d->ntaps * d->Cin;
    {
        const int64_t xb = (int64_t)d->B * d->inH * d->inW * ((d->flags & LOANS_F_DENSE) ? 1 : d->Cin) * 4;
        const int64_t gb = (int64_t)d->B * d->outH * d->outW * d->Cout * ((d->flags & LOANS_F_GY_BF16) ? 2 : 4);
        if (xb >= 0xFFFFFFF0ll || gb >= 0xFFFFFFF0ll) return LOANS_ERANGE;
    }
    const bool small = (d->Cout <= 64) || (Ktot <= 64);
    int tile = d->tile;
    if (tile == 0) tile = small ? LOANS_TILE_64x64 : LOANS_TILE_128x128;
    if (tile == LOANS_TILE_STEM) return bf16 ? LOANS_EINVAL : conv_check_stem7_wgrad(d, misaligned);
    if (tile == LOANS_TILE_64x64 || tile == LOANS_TILE_128x128 || tile == LOANS_TILE_64x128) {
        const bool relu = d->flags & LOANS_F_RELU_IN;
        if ((d->flags & LOANS_F_GY_BF16) && (relu || !bf16)) return LOANS_EINVAL;
        return LOANS_OK;
    }
    if (tile == LOANS_TILE_WGHALO_64) return (bf16 || !conv_wgrad_halo32_covers(d)) ? LOANS_EINVAL : LOANS_OK;
    return LOANS_EINVAL;
}

inline int conv_check_wgrad_f32(const loans_igemm_desc* d, unsigned have, unsigned misaligned) { return conv_check_wgrad32(d, have, misaligned, 0); }
inline int conv_check_wgrad_bf16_f32(const loans_igemm_desc* d, unsigned have, unsigned misaligned) { return conv_check_wgrad32(d, have, misaligned, 1); }

// ---- igemm_bf16.hip ---------------------------------------------------------------------------------------------------------
// loans_igemm_bf16s, loans_igemm_bf16s_splitk (CONV_P_PARTIAL in `have`, `splits`) and the stacked GEMM of
// loans_igemm_pair_bf16s (pair: Cout = 2 x the channels of either convolution, CONV_P_STATS2 = the second one's statistics)
inline int conv_check_igemm16(const loans_igemm_desc* d, unsigned have, unsigned misaligned, int splits = 1, bool pair = false) {
    const bool partial = have & CONV_P_PARTIAL;
    if (!d || !(have & CONV_P_IN) || !(have & CONV_P_W) || (!(have & CONV_P_OUT) && !partial)) return LOANS_EINVAL;
    if (partial && (d->flags & ~(LOANS_F_RELU_IN | LOANS_F_DENSE))) return LOANS_EINVAL;      // raw partial sums only
    if (d->B <= 0 || d->inH <= 0 || d->inW <= 0 || d->Cin <= 0 || (d->Cin & 7)) return LOANS_EINVAL;
    if (d->outH <= 0 || d->outW <= 0 || d->Cout <= 0 || (d->Cout & 7)) return LOANS_EINVAL;
    if (d->gridH <= 0 || d->gridW <= 0 || d->osy <= 0 || d->osx <= 0 || d->isy <= 0 || d->isx <= 0) return LOANS_EINVAL;
    if (d->oy0 < 0 || d->ox0 < 0) return LOANS_EINVAL;
    if ((d->gridH - 1) * d->osy + d->oy0 >= d->outH) return LOANS_EINVAL;
    if ((d->gridW - 1) * d->osx + d->ox0 >= d->outW) return LOANS_EINVAL;
    if (d->ntaps < 1 || d->ntaps > LOANS_MAX_TAPS) return LOANS_EINVAL;
    const bool dense = d->flags & LOANS_F_DENSE;
    if (!dense && d->ntaps > 32) return LOANS_EINVAL;       // the kernel keeps one 32-bit tap mask per tile row
    if (dense) {
        // no bounds masks in this mode: every K-row of every grid pixel has to lie inside its input row; rows and row
        // steps must keep the 16-byte loads 4-byte aligned (even element counts)
        if ((d->inW & 1) || (d->isx & 1)) return LOANS_EINVAL;
        for (int t = 0; t < d->ntaps; ++t) {
            if (d->dy[t] < 0 || d->dx[t] < 0 || (d->dx[t] & 1)) return LOANS_EINVAL;
            if ((d->gridH - 1) * d->isy + d->dy[t] >= d->inH) return LOANS_EINVAL;
            if ((d->gridW - 1) * d->isx + d->dx[t] + d->Cin > d->inW) return LOANS_EINVAL;
        }
    }
    if ((d->flags & LOANS_F_BIAS) && !(have & CONV_P_BIAS)) return LOANS_EINVAL;
    // the BN + ReLU in front of the convolution on load: the VGPR-fed 1 x 1 kernels only, `bias` = its [scale | shift]
    if ((d->flags & LOANS_F_AFFINE_IN) && (d->tile != LOANS_TILE_PW || !(have & CONV_P_BIAS) || partial || pair || (d->flags & ~(LOANS_F_AFFINE_IN | LOANS_F_STATS))))
        return LOANS_EINVAL;
    if ((d->flags & LOANS_F_STATS) && !(have & CONV_P_STATS)) return LOANS_EINVAL;
    if (d->flags & LOANS_F_BNSUMS) {        // a data gradient's epilogue takes the sums of the BN below it: nothing else rides along
        if (!(have & CONV_P_REF) || !(have & CONV_P_BIAS) || !(have & CONV_P_STATS) || partial || pair) return LOANS_EINVAL;
        if (d->flags & (LOANS_F_BIAS | LOANS_F_STATS | LOANS_F_MASK | LOANS_F_ADDEND | LOANS_F_ADDEND_MASK | LOANS_F_DENSE)) return LOANS_EINVAL;
    }
    if ((d->flags & (LOANS_F_MASK | LOANS_F_ADDEND_MASK)) && !(have & CONV_P_REF)) return LOANS_EINVAL;
    if ((d->flags & LOANS_F_ADDEND_MASK) && !(d->flags & LOANS_F_ADDEND)) return LOANS_EINVAL;
    if ((d->flags & LOANS_F_ADDEND) && !(have & CONV_P_ADDEND)) return LOANS_EINVAL;
    const int64_t lim = (int64_t)1 << 31;
    if ((int64_t)d->B * d->gridH * d->gridW >= lim) return LOANS_ERANGE;
    const int M = d->B * d->gridH * d->gridW;
    const int Ktot = d->ntaps * d->Cin;
    if (pair) {                 // `d` describes the stacked GEMM: Cout = 2 x the channels of either convolution
        if (partial || (d->Cout & 63) || (d->flags & ~(LOANS_F_STATS | LOANS_F_RELU_IN))) return LOANS_EINVAL;
        if ((d->flags & LOANS_F_STATS) && !(have & CONV_P_STATS2)) return LOANS_EINVAL;
    }
    unsigned in_bytes, w_bytes;
    {
        const int64_t ib = (int64_t)d->B * d->inH * d->inW * (dense ? 1 : d->Cin) * 2;
        const int64_t wb = (int64_t)d->Cout * Ktot * 2;
        const int64_t ob = (int64_t)d->B * d->outH * d->outW * d->Cout * 2;
        if (ib >= 0xFFFFFFF0ll || wb >= 0xFFFFFFF0ll || ob >= 0xFFFFFFF0ll) return LOANS_ERANGE;   // 32-bit buffer offsets
        in_bytes = (unsigned)ib; w_bytes = (unsigned)wb;
    }
    int tile = d->tile;
    if (tile == 0) {
        const int64_t big = (int64_t)((M + 127) / 128) * ((d->Cout + 127) / 128);
        tile = d->Cout <= 64 ? LOANS_TILE_128x64 : (big >= 512 ? LOANS_TILE_128x128 : LOANS_TILE_64x64);
    }
    const bool halo_tile = (tile >= LOANS_TILE_HALO_128 && tile <= LOANS_TILE_WS64) || tile == LOANS_TILE_HALO_256x128 || tile == LOANS_TILE_HALO_256x256 || tile == LOANS_TILE_WSW64;
    if (partial && halo_tile) return LOANS_EINVAL;          // the halo tiles have no split-K form
    if (pair && (tile == LOANS_TILE_STEM || halo_tile)) return LOANS_EINVAL;
    if (tile == LOANS_TILE_STEM) {          // the dense RGB stem as a direct convolution (stem.hip)
        if (partial || splits > 1) return LOANS_EINVAL;
        return conv_check_stem7_bf16(d, misaligned, 0);
    }
    if (tile == LOANS_TILE_PW) {            // short-K 1 x 1 convolutions, operands never in LDS (pw_bf16.hip); w in fragment order
        if (partial || splits > 1 || pair) return LOANS_EINVAL;
        return conv_check_pw16(d, (have & CONV_P_STATS) | (((d->flags & LOANS_F_AFFINE_IN) && (have & CONV_P_BIAS)) ? CONV_P_AFFINE : 0u));
    }
    switch (tile) {
        case LOANS_TILE_128x128: case LOANS_TILE_128x64: case LOANS_TILE_64x64: case LOANS_TILE_256x64:
        case LOANS_TILE_128x128 | LOANS_TILE_DEEP: case LOANS_TILE_128x64 | LOANS_TILE_DEEP: case LOANS_TILE_64x64 | LOANS_TILE_DEEP:
        case LOANS_TILE_256x128: case LOANS_TILE_256x256:
            return LOANS_OK;
        case LOANS_TILE_256x256PP: case LOANS_TILE_256x256PP16:      // (igemm16_pp.h)
            return (dense || partial) ? LOANS_EINVAL : LOANS_OK;
        case LOANS_TILE_HALO_128: case LOANS_TILE_HALO_128x64: case LOANS_TILE_HALO_256x64: case LOANS_TILE_HALO_128x64S:
        case LOANS_TILE_HALO_256x128: case LOANS_TILE_HALO_256x256: case LOANS_TILE_WSW64: case LOANS_TILE_WS64:
            return conv_check_halo16(d, tile, in_bytes, w_bytes);
        default: return LOANS_EINVAL;
    }
}

inline int conv_check_igemm_bf16s(const loans_igemm_desc* d, unsigned have, unsigned misaligned) {
    if (!(have & CONV_P_OUT)) return LOANS_EINVAL;
    return conv_check_igemm16(d, have & ~CONV_P_PARTIAL, misaligned);
}

// `d` describes convolution a; *stacked = the descriptor of the GEMM with 2 x Cout columns
inline int conv_check_igemm_pair_bf16s(const loans_igemm_desc* d, unsigned have, unsigned misaligned, loans_igemm_desc* stacked) {
    if (!d || !(have & CONV_P_OUT) || d->Cout <= 0 || (d->Cout & 31)) return LOANS_EINVAL;
    *stacked = *d;
    stacked->Cout = 2 * d->Cout;
    return conv_check_igemm16(stacked, have & ~(CONV_P_PARTIAL | CONV_P_BIAS | CONV_P_REF | CONV_P_ADDEND), misaligned, 1, true);
}

inline int conv_check_igemm_bf16s_splitk(const loans_igemm_desc* d, unsigned have, unsigned misaligned, int splits) {
    if (!(have & CONV_P_PARTIAL) || splits < 1 || splits > 64) return LOANS_EINVAL;
    return conv_check_igemm16(d, have & (CONV_P_IN | CONV_P_W | CONV_P_PARTIAL), misaligned, splits);
}

// *nblk = blocks of the launch
inline int conv_check_finalize_bf16(unsigned have, int flags, int64_t rows, int Cout, int64_t* nblk = nullptr) {
    if (!(have & CONV_P_PARTIAL) || !(have & CONV_P_OUT) || rows <= 0 || Cout <= 0 || (Cout & 7)) return LOANS_EINVAL;
    const int C8 = Cout / 8;
    if (C8 > 256 || 256 % C8) return LOANS_EINVAL;          // the thread map: Cout / 8 divides 256
    if ((flags & LOANS_F_BIAS) && !(have & CONV_P_BIAS)) return LOANS_EINVAL;
    if ((flags & LOANS_F_STATS) && !(have & CONV_P_STATS)) return LOANS_EINVAL;
    if ((flags & (LOANS_F_MASK | LOANS_F_ADDEND_MASK)) && !(have & CONV_P_REF)) return LOANS_EINVAL;
    if ((flags & LOANS_F_ADDEND) && !(have & CONV_P_ADDEND)) return LOANS_EINVAL;
    if (flags & ~(LOANS_F_BIAS | LOANS_F_STATS | LOANS_F_MASK | LOANS_F_ADDEND | LOANS_F_ADDEND_MASK)) return LOANS_EINVAL;
    const int rows_per_block = 256 / C8 * 8;
    const int64_t n = (rows + rows_per_block - 1) / rows_per_block;
    if (n >= ((int64_t)1 << 31)) return LOANS_ERANGE;
    if (nblk) *nblk = n;
    return LOANS_OK;
}

// loans_wgrad_bf16s, loans_wgrad_bf16s_ws (need_ws), loans_wgrad_bf16s_affine_ws (need_ws, need_affine) and
// loans_wgrad_bf16s_ws_floats (plan_only: no pointers), up to the slab plan
inline int conv_check_wgrad_bf16s(const loans_igemm_desc* d, unsigned have, unsigned misaligned, bool plan_only = false,
                              bool need_ws = false, bool need_affine = false) {
    if (need_ws && !(have & CONV_P_WS)) return LOANS_EINVAL;
    if (need_affine && (!(have & CONV_P_AFFINE) || !d || !(d->flags & LOANS_F_AFFINE_IN))) return LOANS_EINVAL;
    if (!d || (!plan_only && (!(have & CONV_P_X) || !(have & CONV_P_GY) || !(have & CONV_P_DW)))) return LOANS_EINVAL;
    if (d->B <= 0 || d->inH <= 0 || d->inW <= 0 || d->Cin <= 0 || (d->Cin & 7)) return LOANS_EINVAL;
    if (d->outH <= 0 || d->outW <= 0 || d->Cout <= 0 || (d->Cout & 7)) return LOANS_EINVAL;
    if (d->gridH <= 0 || d->gridW <= 0 || d->osy <= 0 || d->osx <= 0 || d->isy <= 0 || d->isx <= 0) return LOANS_EINVAL;
    if (d->oy0 < 0 || d->ox0 < 0) return LOANS_EINVAL;
    if ((d->gridH - 1) * d->osy + d->oy0 >= d->outH) return LOANS_EINVAL;
    if ((d->gridW - 1) * d->osx + d->ox0 >= d->outW) return LOANS_EINVAL;
    if (d->ntaps < 1 || d->ntaps > LOANS_MAX_TAPS) return LOANS_EINVAL;
    // the kernel reads the gradient at grid pixel m itself and keeps the input offset incrementally with 24-bit multiplies
    if (d->osy != 1 || d->osx != 1 || d->oy0 || d->ox0 || d->outH != d->gridH || d->outW != d->gridW) return LOANS_EINVAL;
    {
        const int64_t uc = (d->flags & LOANS_F_DENSE) ? 1 : d->Cin;
        const int64_t xr = ((int64_t)d->isy * d->inW - (int64_t)d->isx * d->gridW) * uc * 2;
        const int64_t xi = ((int64_t)d->inH - (int64_t)d->isy * d->gridH) * d->inW * uc * 2;
        const int64_t lim24 = (int64_t)1 << 23;
        if (xr <= -lim24 || xr >= lim24 || xi <= -lim24 || xi >= lim24) return LOANS_ERANGE;
        if (d->gridW >= lim24 || d->gridH >= lim24) return LOANS_ERANGE;
    }
    const bool dense = d->flags & LOANS_F_DENSE;
    if (dense) {            // as in loans_igemm_bf16s
        if ((d->inW & 1) || (d->isx & 1)) return LOANS_EINVAL;
        for (int t = 0; t < d->ntaps; ++t) {
            if (d->dy[t] < 0 || d->dx[t] < 0 || (d->dx[t] & 1)) return LOANS_EINVAL;
            if ((d->gridH - 1) * d->isy + d->dy[t] >= d->inH) return LOANS_EINVAL;
            if ((d->gridW - 1) * d->isx + d->dx[t] + d->Cin > d->inW) return LOANS_EINVAL;
        }
    }
    if ((int64_t)d->B * d->gridH * d->gridW >= ((int64_t)1 << 31)) return LOANS_ERANGE;
    const int Ktot = d->ntaps * d->Cin;
    if (d->flags & LOANS_F_AFFINE_IN) {     // 1 x 1 / 1 convolutions on the GEMM tiles only; x = the BN's input, affine = [scale | shift][Cin]
        if (plan_only) { /* the slab count does not depend on it */ }
        else if (!(have & CONV_P_AFFINE)) return LOANS_EINVAL;
        if (d->ntaps != 1 || d->dy[0] != 0 || d->dx[0] != 0 || d->isy != 1 || d->isx != 1 || (d->flags & ~LOANS_F_AFFINE_IN)) return LOANS_EINVAL;
    }
    {
        const int64_t xb = (int64_t)d->B * d->inH * d->inW * (dense ? 1 : d->Cin) * 2;
        const int64_t gb = (int64_t)d->B * d->outH * d->outW * d->Cout * 2;
        if (xb >= 0xFFFFFFF0ll || gb >= 0xFFFFFFF0ll) return LOANS_ERANGE;
    }
    int tile = d->tile;
    if (tile == 0) tile = (d->Cout <= 64) ? (Ktot <= 64 ? LOANS_TILE_64x64 : LOANS_TILE_64x128) : LOANS_TILE_128x128;
    const bool halo = tile == LOANS_TILE_WGHALO_64 || tile == LOANS_TILE_WGHALO_128;
    if (halo && (d->flags & LOANS_F_AFFINE_IN)) return LOANS_EINVAL;
    if (tile == LOANS_TILE_STEM)
        return (!conv_stem7_wgrad_bf16_covers(d) || (misaligned & (CONV_P_X | CONV_P_GY | CONV_P_WS))) ? LOANS_EINVAL : LOANS_OK;
    if (halo) return conv_wgrad_halo16_covers(d, tile) ? LOANS_OK : LOANS_EINVAL;
    if (tile == LOANS_TILE_64x64 || tile == LOANS_TILE_128x128 || tile == LOANS_TILE_64x128 || tile == LOANS_TILE_256x256) return LOANS_OK;
    return LOANS_EINVAL;
}
