// Host-side rules of the convolution launchers (not part of the C ABI): what makes a loans_igemm_desc launchable, each rule once,
// and one check per entry point.  Plain C++ as well as HIP, no HIP calls or types.  A check sees the descriptor(s), the integer
// arguments and WHICH pointers are there (CONV_P_* bits; `misaligned`: the same bits for address & 15), never an address; it
// returns LOANS_OK / _EINVAL / _ERANGE before the entry fills an argument struct.  What needs the device (CU counts, LDS limits,
// the stem's row plans, slab planning) stays with the launchers.  Products and sums of descriptor fields are taken in int64_t,
// factor by factor where three could pass 2^63.  tests/conv_desc/test_desc_cpu.py owns these rules.
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
constexpr int CONV_F_EPILOGUE = LOANS_F_BIAS | LOANS_F_STATS | LOANS_F_MASK | LOANS_F_ADDEND | LOANS_F_ADDEND_MASK;
constexpr int64_t CONV_BUFFER_LIMIT = 0xFFFFFFF0ll, CONV_INDEX_LIMIT = (int64_t)1 << 31;       // 32-bit buffer offsets, int indices

// ---- shared predicates --------------------------------------------------------------------------------------------------------
// a * b for a >= 0 and 0 <= b < 2^31, saturating at 2^32 (every limit here is at most that): no step can overflow
inline int64_t conv_mul(int64_t a, int64_t b) { const int64_t cap = (int64_t)1 << 32; return a >= cap || a * b >= cap ? cap : a * b; }
inline int64_t conv_elems(int64_t b, int64_t h, int64_t w, int64_t c) { return conv_mul(conv_mul(conv_mul(b, h), w), c); }
inline int64_t conv_in_channels(const loans_igemm_desc* d) { return (d->flags & LOANS_F_DENSE) ? 1 : d->Cin; }    // per unit of inW

// C/4 float4 groups must tile 256-thread blocks: a divisor of 256, or a multiple of 256 (slabs)
inline bool reduce_channels_ok(int C) {
    const int c4 = C / 4;
    return C >= 4 && !(C & 3) && (c4 <= 256 ? (256 % c4 == 0) : (c4 % 256 == 0));
}

// positive sizes, channel alignment (powers of two), grid inside the output, tap count (taps32: <= 32 when not dense -- the bf16
// kernels keep one 32-bit tap mask per tile row); count_range: the fp32 arm's 31-bit element counts
inline int conv_check_shape(const loans_igemm_desc* d, int cin_align, int cout_align, bool count_range, bool taps32) {
    if (!d || d->B <= 0 || d->inH <= 0 || d->inW <= 0 || d->Cin <= 0 || (d->Cin & (cin_align - 1))) return LOANS_EINVAL;
    if (d->outH <= 0 || d->outW <= 0 || d->Cout <= 0 || (d->Cout & (cout_align - 1)) || d->oy0 < 0 || d->ox0 < 0) return LOANS_EINVAL;
    if (d->gridH <= 0 || d->gridW <= 0 || d->osy <= 0 || d->osx <= 0 || d->isy <= 0 || d->isx <= 0) return LOANS_EINVAL;
    if ((int64_t)(d->gridH - 1) * d->osy + d->oy0 >= d->outH || (int64_t)(d->gridW - 1) * d->osx + d->ox0 >= d->outW) return LOANS_EINVAL;
    if (d->ntaps < 1 || d->ntaps > LOANS_MAX_TAPS || (taps32 && !(d->flags & LOANS_F_DENSE) && d->ntaps > 32)) return LOANS_EINVAL;
    const int64_t lim = CONV_INDEX_LIMIT;
    if (count_range && (conv_elems(d->B, d->inH, d->inW, conv_in_channels(d)) >= lim || conv_elems(d->B, d->outH, d->outW, d->Cout) >= lim ||
                        conv_elems(d->B, d->gridH, d->gridW, 1) >= lim || conv_elems(d->ntaps, d->Cin, d->Cout, 1) >= lim))
        return LOANS_ERANGE;
    return LOANS_OK;
}

// LOANS_F_DENSE has no bounds masks: every K-row of every grid pixel has to lie inside its input row.  even: rows and row
// steps keep the bf16 arm's 16-byte loads 4-byte aligned (even element counts)
inline int conv_check_dense_window(const loans_igemm_desc* d, bool even) {
    if (!(d->flags & LOANS_F_DENSE)) return LOANS_OK;
    if (even && ((d->inW & 1) || (d->isx & 1))) return LOANS_EINVAL;
    for (int t = 0; t < d->ntaps; ++t) {
        if (d->dy[t] < 0 || d->dx[t] < 0 || (even && (d->dx[t] & 1))) return LOANS_EINVAL;
        if ((int64_t)(d->gridH - 1) * d->isy + d->dy[t] >= d->inH || (int64_t)(d->gridW - 1) * d->isx + d->dx[t] + d->Cin > d->inW) return LOANS_EINVAL;
    }
    return LOANS_OK;
}

// the epilogue flags against the pointers they read; nothing outside `allowed`.  lone_addend_mask: ADDEND_MASK without ADDEND passes
// (loans_igemm_finalize_bf16 ignores it).  LOANS_F_BNSUMS (the sums of the BN below a data gradient) takes ref, bias, stats, nothing else
inline int conv_check_epilogue(int flags, int allowed, unsigned have, bool lone_addend_mask = false) {
    if ((flags & ~allowed) || ((flags & LOANS_F_BIAS) && !(have & CONV_P_BIAS)) || ((flags & LOANS_F_STATS) && !(have & CONV_P_STATS))) return LOANS_EINVAL;
    if ((flags & (LOANS_F_MASK | LOANS_F_ADDEND_MASK)) && !(have & CONV_P_REF)) return LOANS_EINVAL;
    if ((flags & LOANS_F_ADDEND_MASK) && !(flags & LOANS_F_ADDEND) && !lone_addend_mask) return LOANS_EINVAL;
    if ((flags & LOANS_F_ADDEND) && !(have & CONV_P_ADDEND)) return LOANS_EINVAL;
    const unsigned sums = CONV_P_REF | CONV_P_BIAS | CONV_P_STATS;
    return ((flags & LOANS_F_BNSUMS) && ((have & sums) != sums || (flags & (CONV_F_EPILOGUE | LOANS_F_DENSE)))) ? LOANS_EINVAL : LOANS_OK;
}

// bytes of the gathered tensor, the weights ([Cout][ntaps][Cin], elements as wide as the input's; 0 without `weights`) and the
// output, each below `limit`: they become the kernels' buffer sizes
struct ConvBytes { unsigned in, w, out; };
inline int conv_tensor_bytes(const loans_igemm_desc* d, int in_elem_bytes, int out_elem_bytes, int64_t limit, ConvBytes* b, bool weights = true) {
    const int64_t ib = conv_mul(conv_elems(d->B, d->inH, d->inW, conv_in_channels(d)), in_elem_bytes);
    const int64_t wb = weights ? conv_mul(conv_elems(d->Cout, d->ntaps, d->Cin, 1), in_elem_bytes) : 0;
    const int64_t ob = conv_mul(conv_elems(d->B, d->outH, d->outW, d->Cout), out_elem_bytes);
    if (ib >= limit || wb >= limit || ob >= limit) return LOANS_ERANGE;
    b->in = (unsigned)ib; b->w = (unsigned)wb; b->out = (unsigned)ob;
    return LOANS_OK;
}

// an output row is a grid pixel / an input pixel step is one pixel
inline bool conv_plain_output(const loans_igemm_desc* d) { return d->osy == 1 && d->osx == 1 && !d->oy0 && !d->ox0 && d->outH == d->gridH && d->outW == d->gridW; }
inline bool conv_unit_stride(const loans_igemm_desc* d) { return d->isy == 1 && d->isx == 1; }

// the taps are a row-major, ascending ny x nx grid with its first tap in [lo, 0] on both axes
inline bool conv_taps_are(const loans_igemm_desc* d, int ny, int nx, int lo) {
    if (d->ntaps != ny * nx) return false;
    const TapGrid g = detect_tap_grid(d);
    return g.nx == nx && g.ny == ny && g.sdy == 1 && g.sdx == 1 && g.dy0 >= lo && g.dy0 <= 0 && g.dx0 >= lo && g.dx0 <= 0;
}

// ---- stem.hip: LOANS_TILE_STEM ------------------------------------------------------------------------------------------------
// the dense 7x7 / 2, Cout = 64 forward geometry: 7 rows of 24 elements per output pixel, whole windows inside even-sized frames
inline bool conv_stem7_geometry(const loans_igemm_desc* d) {
    if (d->ntaps != 7 || d->Cin != 24 || d->Cout != 64 || d->isy != 2 || d->isx != 6) return false;
    if ((d->inW & 1) || (d->inH & 1) || !conv_taps_are(d, 7, 1, 0) || !conv_plain_output(d)) return false;
    return 2 * ((int64_t)d->gridH - 1) + 7 <= d->inH && 6 * ((int64_t)d->gridW - 1) + 24 <= d->inW;
}

// a direct stem launch (up to the kernels' LDS limits): flags `required`, maybe some of `optional`; the pointers in `aligned` on 16-byte boundaries
inline int conv_check_stem7(const loans_igemm_desc* d, int required, int optional, unsigned misaligned, unsigned aligned) {
    if ((d->flags & required) != required || (d->flags & ~(required | optional)) || !conv_stem7_geometry(d) || (misaligned & aligned)) return LOANS_EINVAL;
    return (conv_elems(d->B, d->inH, d->inW, 1) >= CONV_INDEX_LIMIT || conv_elems(d->B, d->gridH, d->gridW, 64) >= CONV_INDEX_LIMIT) ? LOANS_ERANGE : LOANS_OK;
}
// of loans_wgrad_bf16s: rows of whole 12-byte cells, Wo + 3 of them (the kernel's own tile limits stay in stem.hip)
inline int conv_stem7_wgrad_bf16_covers(const loans_igemm_desc* d) {
    return d->flags == LOANS_F_DENSE && conv_stem7_geometry(d) && !(d->gridW & 15) && d->inW == 6 * ((int64_t)d->gridW + 3);
}

// ---- halo_bf16.hip, pw_bf16.hip, wgrad_halo_*.hip -----------------------------------------------------------------------------
// 1 if the descriptor is a geometry the halo kernels cover (conv_check_igemm16 has validated everything else)
inline int conv_halo16_covers(const loans_igemm_desc* d, int tile) {
    if ((d->flags & LOANS_F_DENSE) || ((d->flags & LOANS_F_BNSUMS) && tile == LOANS_TILE_WS64)) return 0;       // ws8_kernel's epilogue does not take the BN sums
    if (!conv_unit_stride(d) || !conv_plain_output(d) || d->Cin % 64 || d->ntaps > 9) return 0;
    if ((tile == LOANS_TILE_HALO_256x64 || tile == LOANS_TILE_HALO_128x64S) && d->Cin != 64) return 0;
    if ((tile == LOANS_TILE_WS64 || tile == LOANS_TILE_WSW64) && (d->Cin != 64 || d->Cout > 64 || d->ntaps != 9 || (d->flags & LOANS_F_RELU_IN))) return 0;
    const TapGrid g = detect_tap_grid(d);       // a grid of at most 3 x 3, either direction (nine taps: 3 x 3)
    return g.nx > 0 && g.nx <= 3 && g.ny <= 3;
}

// LOANS_TILE_PW covers: 1 x 1 / 1 forward (grid = input = output), Cin 64 | 128 with Cout % 64 == 0 up to 512 or Cin 256 with Cout % 128 == 0 up to 1024
inline int conv_pw16_covers(const loans_igemm_desc* d) {
    if (!conv_taps_are(d, 1, 1, 0) || !conv_unit_stride(d) || !conv_plain_output(d) || d->gridH != d->inH || d->gridW != d->inW) return 0;
    const int n = d->Cin == 256 ? 128 : 64;         // the column tile; at most 8 of them
    if ((d->Cin != 64 && d->Cin != 128 && d->Cin != 256) || d->Cout % n != 0 || d->Cout < n || d->Cout > 8 * n) return 0;
    return !(d->flags & ~(LOANS_F_STATS | LOANS_F_AFFINE_IN));
}
// loans_pw16_launch; `have`: CONV_P_STATS, and CONV_P_AFFINE for the [scale | shift] table
inline int conv_check_pw16(const loans_igemm_desc* d, unsigned have) {
    if (!conv_pw16_covers(d)) return LOANS_EINVAL;
    if (conv_elems(d->B, d->gridH, d->gridW, 1) > 0x7FFFFFFF - 64) return LOANS_ERANGE;
    return (((d->flags & LOANS_F_STATS) && !(have & CONV_P_STATS)) || ((d->flags & LOANS_F_AFFINE_IN) && !(have & CONV_P_AFFINE))) ? LOANS_EINVAL : LOANS_OK;
}

// LOANS_TILE_WGHALO_* cover: stride-1 forward geometry, row-major 3 x 3 taps (any padding), Cin % 64 == 0, Cout % cout_multiple == 0, not dense
inline int conv_wgrad_halo_covers(const loans_igemm_desc* d, int cout_multiple) {
    if ((d->flags & ~LOANS_F_RELU_IN) || !conv_unit_stride(d) || !conv_plain_output(d) || d->inH != d->outH || d->inW != d->outW) return 0;
    return !(d->Cin % 64) && !(d->Cout % cout_multiple) && conv_taps_are(d, 3, 3, -2);
}

// ---- igemm.hip ----------------------------------------------------------------------------------------------------------------
// loans_igemm_f32 / _bf16_f32 (bf16 = 1), a pair launch (second convolution: pair_cout channels) or a class launch (ncls >= 2:
// descs[0] is `d`; bit c of w_have = the weights of class c are there)
inline int conv_check_igemm32(const loans_igemm_desc* d, unsigned have, unsigned misaligned, int bf16, bool pair = false,
                              int pair_cout = 0, int ncls = 0, const loans_igemm_desc* descs = nullptr, unsigned w_have = 0) {
    const bool mc = ncls > 0;
    int rc = conv_check_shape(d, 4, 1, true, false);
    if (rc || (rc = conv_check_dense_window(d, false))) return rc;
    if (!(have & CONV_P_IN) || !(have & CONV_P_W) || !(have & CONV_P_OUT) || (d->Cout & 3)) return LOANS_EINVAL;
    if (conv_check_epilogue(d->flags, ~0, have) || ((d->flags & LOANS_F_BNSUMS) && (pair || mc || (d->tile & 0xEF) == LOANS_TILE_FINETAIL))) return LOANS_EINVAL;
    if ((d->flags & LOANS_F_OUT_BF16) && (d->flags & (LOANS_F_MASK | LOANS_F_ADDEND | LOANS_F_ADDEND_MASK | LOANS_F_BNSUMS))) return LOANS_EINVAL;
    ConvBytes b;
    if ((rc = conv_tensor_bytes(d, 4, (d->flags & LOANS_F_OUT_BF16) ? 2 : 4, CONV_BUFFER_LIMIT, &b))) return rc;
    loans_igemm_desc d2 = *d;       // the second convolution of a pair
    d2.Cout = pair_cout;
    if (pair && (rc = conv_tensor_bytes(&d2, 4, 4, CONV_BUFFER_LIMIT, &b))) return rc;
    if (mc) {
        // the classes differ in their grid, their output phase and their taps; image, strides, channels and flags are shared
        if (pair || bf16 || ncls < 2 || ncls > LOANS_MAX_CLASSES || (d->flags & (LOANS_F_DENSE | LOANS_F_STATS | LOANS_F_BIAS))) return LOANS_EINVAL;
        for (int c = 0; c < ncls; ++c) {
            const loans_igemm_desc* e = descs + c;
            if ((rc = conv_check_shape(e, 4, 1, true, false))) return rc;      // (not dense: d is not, and the flags agree)
            if (!((w_have >> c) & 1) || e->ntaps > LOANS_MAX_CLS_TAPS) return LOANS_EINVAL;
            if (e->B != d->B || e->inH != d->inH || e->inW != d->inW || e->Cin != d->Cin || e->outH != d->outH || e->outW != d->outW ||
                e->Cout != d->Cout || e->osy != d->osy || e->osx != d->osx || e->isy != d->isy || e->isx != d->isx || e->flags != d->flags)
                return LOANS_EINVAL;
        }
    }
    int tile = d->tile;
    const int t = tile & ~LOANS_TILE_DMA;   // a class launch names its tile shape
    if (mc && t != LOANS_TILE_128x128 && t != LOANS_TILE_128x64 && t != LOANS_TILE_64x64 && t != LOANS_TILE_256x64) return LOANS_EINVAL;
    if (pair && ((tile >> 8) || (tile & 0xFF) == LOANS_TILE_SPLIT)) return LOANS_EINVAL;
    const int splits = (tile >> 8) & 0xFF;  // LOANS_TILE_SPLITK(s)
    tile &= 0xFF;
    if (tile & LOANS_TILE_POSMAJOR) {       // image-strided row tiles: the per-tap loader of the 64x64 tile, an ordinary fp32 launch of whole images
        if (bf16 || pair || mc || (d->tile >> 8) || (tile & ~(LOANS_TILE_DMA | LOANS_TILE_POSMAJOR)) != LOANS_TILE_64x64) return LOANS_EINVAL;
        return ((d->Cin & 31) || (d->flags & (LOANS_F_DENSE | LOANS_F_OUT_BF16)) || d->B < 64 || detect_tap_grid(d).nx == 0) ? LOANS_EINVAL : LOANS_OK;
    }
    if (splits > 1 && (bf16 || (d->flags & ~(LOANS_F_DENSE | LOANS_F_RELU_IN)) || tile == LOANS_TILE_SPLIT))
        return LOANS_EINVAL;                // raw partial sums only: the epilogue flags belong to loans_igemm_finalize_f32
    const bool dma = tile & LOANS_TILE_DMA;
    if (dma && bf16) return LOANS_EINVAL;
    switch (tile & ~LOANS_TILE_DMA) {
        case 0: case LOANS_TILE_SPLIT:
        case LOANS_TILE_128x128: case LOANS_TILE_128x64: case LOANS_TILE_64x64: case LOANS_TILE_256x64: return LOANS_OK;
        case LOANS_TILE_STEM:               // the dense RGB stem as a direct convolution (stem.hip)
            if (pair || splits > 1 || dma) return LOANS_EINVAL;
            return conv_check_stem7(d, LOANS_F_DENSE | (bf16 ? LOANS_F_OUT_BF16 : 0), LOANS_F_BIAS | LOANS_F_STATS, misaligned,
                                    CONV_P_IN | CONV_P_W | (bf16 ? CONV_P_OUT : 0u));      // (bf16: the output is a bf16 tensor)
        case LOANS_TILE_FINETAIL:           // forward geometry, bias and statistics from the finalize pass (its thread map)
            if (pair || bf16 || splits > 1 || !conv_plain_output(d) || !reduce_channels_ok(d->Cout)) return LOANS_EINVAL;
            return (d->flags & (LOANS_F_MASK | LOANS_F_ADDEND | LOANS_F_ADDEND_MASK | LOANS_F_OUT_BF16)) ? LOANS_EINVAL : LOANS_OK;
        default: return LOANS_EINVAL;
    }
}
inline int conv_check_igemm_pair_f32(const loans_igemm_desc* d, unsigned have, unsigned misaligned, int Cout_b) {
    if (!d || !(have & CONV_P_W2) || !(have & CONV_P_OUT2) || Cout_b <= 0 || (Cout_b & 3)) return LOANS_EINVAL;
    if (conv_check_epilogue(d->flags, LOANS_F_STATS | LOANS_F_RELU_IN, (have & CONV_P_STATS2) ? CONV_P_STATS : 0u)) return LOANS_EINVAL;
    return conv_check_igemm32(d, have & ~(CONV_P_BIAS | CONV_P_REF | CONV_P_ADDEND), misaligned, 0, true, Cout_b);
}
// have_w: the array of weight pointers is there; bit c of w_have: so is its entry c
inline int conv_check_igemm_classes_f32(const loans_igemm_desc* descs, int n, unsigned have, unsigned misaligned, bool have_w, unsigned w_have) {
    if (!descs || !have_w || n < 1) return LOANS_EINVAL;
    have = (have & ~(CONV_P_W | CONV_P_BIAS | CONV_P_STATS)) | ((w_have & 1) ? CONV_P_W : 0u);
    return conv_check_igemm32(descs, have, misaligned, 0, false, 0, n == 1 ? 0 : n, descs, w_have);
}
inline int conv_check_finalize_f32(unsigned have, int flags, int64_t rows, int C) {
    if (!(have & CONV_P_OUT) || rows <= 0 || !reduce_channels_ok(C)) return LOANS_EINVAL;
    return conv_check_epilogue(flags, CONV_F_EPILOGUE, have);
}

// loans_wgrad_f32 / loans_wgrad_bf16_f32 (bf16 = 1); *b: x is the `in` and gy the `out` of conv_tensor_bytes
inline int conv_check_wgrad32(const loans_igemm_desc* d, unsigned have, unsigned misaligned, int bf16, ConvBytes* b) {
    int rc = conv_check_shape(d, 4, 1, true, false);
    if (rc || (rc = conv_check_dense_window(d, false))) return rc;
    if (!(have & CONV_P_X) || !(have & CONV_P_GY) || !(have & CONV_P_DW) || (d->Cout & 3)) return LOANS_EINVAL;
    if ((rc = conv_tensor_bytes(d, 4, (d->flags & LOANS_F_GY_BF16) ? 2 : 4, CONV_BUFFER_LIMIT, b, false))) return rc;
    switch (d->tile) {
        case 0: case LOANS_TILE_64x64: case LOANS_TILE_128x128: case LOANS_TILE_64x128:      // a bf16 gy: the bf16 MFMA, no relu
            return ((d->flags & LOANS_F_GY_BF16) && ((d->flags & LOANS_F_RELU_IN) || !bf16)) ? LOANS_EINVAL : LOANS_OK;
        case LOANS_TILE_STEM: return bf16 ? LOANS_EINVAL : conv_check_stem7(d, LOANS_F_DENSE, 0, misaligned, CONV_P_X | CONV_P_GY);
        case LOANS_TILE_WGHALO_64: return (bf16 || !conv_wgrad_halo_covers(d, 64)) ? LOANS_EINVAL : LOANS_OK;
        default: return LOANS_EINVAL;
    }
}

// ---- igemm_bf16.hip -----------------------------------------------------------------------------------------------------------
// loans_igemm_bf16s (`have` without CONV_P_PARTIAL), loans_igemm_bf16s_splitk (with it and not CONV_P_OUT; `splits`) and the stacked GEMM of
// loans_igemm_pair_bf16s (pair: Cout = 2 x the channels of either convolution, CONV_P_STATS2 = the second one's statistics)
inline int conv_check_igemm16(const loans_igemm_desc* d, unsigned have, unsigned misaligned, int splits = 1, bool pair = false) {
    const bool partial = have & CONV_P_PARTIAL;
    if (!d || !(have & CONV_P_IN) || !(have & CONV_P_W) || (!(have & CONV_P_OUT) && !partial)) return LOANS_EINVAL;
    if (partial && (splits < 1 || splits > 64 || (d->flags & ~(LOANS_F_RELU_IN | LOANS_F_DENSE)))) return LOANS_EINVAL;      // raw partial sums only
    if (conv_check_shape(d, 8, 8, false, true) || conv_check_dense_window(d, true)) return LOANS_EINVAL;
    // the BN + ReLU in front of the convolution on load: the VGPR-fed 1 x 1 kernels only, `bias` = its [scale | shift]
    if ((d->flags & LOANS_F_AFFINE_IN) && (d->tile != LOANS_TILE_PW || !(have & CONV_P_BIAS) || partial || pair || (d->flags & ~(LOANS_F_AFFINE_IN | LOANS_F_STATS))))
        return LOANS_EINVAL;
    if (conv_check_epilogue(d->flags, ~0, have) || ((d->flags & LOANS_F_BNSUMS) && (partial || pair))) return LOANS_EINVAL;
    if (conv_elems(d->B, d->gridH, d->gridW, 1) >= CONV_INDEX_LIMIT) return LOANS_ERANGE;
    if (pair && (partial || (d->Cout & 63) || (d->flags & ~(LOANS_F_STATS | LOANS_F_RELU_IN)) || ((d->flags & LOANS_F_STATS) && !(have & CONV_P_STATS2))))
        return LOANS_EINVAL;
    ConvBytes b;
    if (int rc = conv_tensor_bytes(d, 2, 2, CONV_BUFFER_LIMIT, &b)) return rc;
    switch (d->tile) {
        case 0: case LOANS_TILE_128x128: case LOANS_TILE_128x64: case LOANS_TILE_64x64: case LOANS_TILE_256x64:
        case LOANS_TILE_128x128 | LOANS_TILE_DEEP: case LOANS_TILE_128x64 | LOANS_TILE_DEEP: case LOANS_TILE_64x64 | LOANS_TILE_DEEP:
        case LOANS_TILE_256x128: case LOANS_TILE_256x256: return LOANS_OK;
        case LOANS_TILE_256x256PP: case LOANS_TILE_256x256PP16:      // (igemm16_pp.h)
            return ((d->flags & LOANS_F_DENSE) || partial) ? LOANS_EINVAL : LOANS_OK;
        case LOANS_TILE_STEM:               // the dense RGB stem as a direct convolution (stem.hip)
            if (partial || pair || splits > 1) return LOANS_EINVAL;     // (LOANS_F_OUT_BF16 is implied here, not set)
            return conv_check_stem7(d, LOANS_F_DENSE, LOANS_F_BIAS | LOANS_F_STATS, misaligned, CONV_P_IN | CONV_P_W | CONV_P_OUT);
        case LOANS_TILE_PW:                 // short-K 1 x 1 convolutions, operands never in LDS (pw_bf16.hip); w in fragment order
            if (partial || splits > 1 || pair) return LOANS_EINVAL;
            return conv_check_pw16(d, (have & CONV_P_STATS) | (((d->flags & LOANS_F_AFFINE_IN) && (have & CONV_P_BIAS)) ? CONV_P_AFFINE : 0u));
        case LOANS_TILE_HALO_128: case LOANS_TILE_HALO_128x64: case LOANS_TILE_HALO_256x64: case LOANS_TILE_HALO_128x64S:
        case LOANS_TILE_HALO_256x128: case LOANS_TILE_HALO_256x256: case LOANS_TILE_WSW64: case LOANS_TILE_WS64:
            if (partial || pair || !conv_halo16_covers(d, d->tile)) return LOANS_EINVAL;        // no split-K form, no pair form
            return conv_tensor_bytes(d, 2, 0, 0x80000000ll, &b);        // input and weight offsets >= 2^31 mean "no load" there; the output keeps the limit above
        default: return LOANS_EINVAL;
    }
}
// `d` describes convolution a; *stacked = the descriptor of the GEMM with 2 x Cout columns
inline int conv_check_igemm_pair_bf16s(const loans_igemm_desc* d, unsigned have, unsigned misaligned, loans_igemm_desc* stacked) {
    if (!d || !(have & CONV_P_OUT) || d->Cout <= 0 || (d->Cout & 31)) return LOANS_EINVAL;
    if (d->Cout > 0x3FFFFFFF) return LOANS_ERANGE;
    *stacked = *d;
    stacked->Cout = 2 * d->Cout;
    return conv_check_igemm16(stacked, have & ~(CONV_P_PARTIAL | CONV_P_BIAS | CONV_P_REF | CONV_P_ADDEND), misaligned, 1, true);
}

// *nblk = blocks of the launch: 8 passes of the 256 / (Cout / 8) rows a block holds
inline int conv_check_finalize_bf16(unsigned have, int flags, int64_t rows, int Cout, int64_t* nblk) {
    if (!(have & CONV_P_PARTIAL) || !(have & CONV_P_OUT) || rows <= 0 || Cout <= 0 || (Cout & 7)) return LOANS_EINVAL;
    const int C8 = Cout / 8;                                // the thread map: Cout / 8 divides 256
    if (C8 > 256 || 256 % C8 || conv_check_epilogue(flags, CONV_F_EPILOGUE, have, true)) return LOANS_EINVAL;
    const int rows_per_block = 256 / C8 * 8;
    const int64_t n = rows / rows_per_block + (rows % rows_per_block != 0);
    if (n >= ((int64_t)1 << 31)) return LOANS_ERANGE;
    *nblk = n;
    return LOANS_OK;
}

// loans_wgrad_bf16s, _ws (need_ws), _affine_ws (need_ws, need_affine) and _ws_floats (plan_only: no pointers), up to the slab plan; *b: x and gy bytes
inline int conv_check_wgrad_bf16s(const loans_igemm_desc* d, unsigned have, unsigned misaligned, bool plan_only, bool need_ws, bool need_affine, ConvBytes* b) {
    if ((need_ws && !(have & CONV_P_WS)) || (need_affine && (!(have & CONV_P_AFFINE) || !d || !(d->flags & LOANS_F_AFFINE_IN)))) return LOANS_EINVAL;
    if (!d || (!plan_only && (!(have & CONV_P_X) || !(have & CONV_P_GY) || !(have & CONV_P_DW)))) return LOANS_EINVAL;
    // the kernel reads the gradient at grid pixel m itself and keeps the input offset incrementally with 24-bit multiplies
    if (conv_check_shape(d, 8, 8, false, false) || !conv_plain_output(d)) return LOANS_EINVAL;
    const int64_t lim24 = (int64_t)1 << 23, uc2 = conv_in_channels(d) * 2;
    auto fits = [&](int64_t v) { return v > -lim24 && v < lim24; };        // (a product of integers fits only if every prefix does)
    const int64_t xr = (int64_t)d->isy * d->inW - (int64_t)d->isx * d->gridW, xi = (int64_t)d->inH - (int64_t)d->isy * d->gridH;
    if (!fits(xr) || !fits(xr * uc2) || !fits(xi) || !fits(xi * d->inW) || !fits(xi * d->inW * uc2) || d->gridW >= lim24 || d->gridH >= lim24) return LOANS_ERANGE;
    if (conv_check_dense_window(d, true)) return LOANS_EINVAL;
    if (conv_elems(d->B, d->gridH, d->gridW, 1) >= CONV_INDEX_LIMIT) return LOANS_ERANGE;
    if (d->flags & LOANS_F_AFFINE_IN) {     // 1 x 1 / 1 convolutions on the GEMM tiles only; x = the BN's input, affine = [scale | shift][Cin]
        if (!plan_only && !(have & CONV_P_AFFINE)) return LOANS_EINVAL;        // (the slab count does not depend on it)
        if (!conv_taps_are(d, 1, 1, 0) || !conv_unit_stride(d) || (d->flags & ~LOANS_F_AFFINE_IN)) return LOANS_EINVAL;
    }
    if (int rc = conv_tensor_bytes(d, 2, 2, CONV_BUFFER_LIMIT, b, false)) return rc;
    switch (d->tile) {
        case 0: case LOANS_TILE_64x64: case LOANS_TILE_128x128: case LOANS_TILE_64x128: case LOANS_TILE_256x256: return LOANS_OK;
        case LOANS_TILE_STEM:
            return (!conv_stem7_wgrad_bf16_covers(d) || (misaligned & (CONV_P_X | CONV_P_GY | CONV_P_WS))) ? LOANS_EINVAL : LOANS_OK;
        case LOANS_TILE_WGHALO_64: case LOANS_TILE_WGHALO_128:
            return ((d->flags & LOANS_F_AFFINE_IN) || !conv_wgrad_halo_covers(d, d->tile == LOANS_TILE_WGHALO_64 ? 64 : 128)) ? LOANS_EINVAL : LOANS_OK;
        default: return LOANS_EINVAL;
    }
}
