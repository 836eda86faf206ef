// Row arithmetic shared by the implicit-GEMM convolution kernels (igemm.hip, igemm_bf16.hip, igemm16_pp.h) and the block
// remaps of every kernel that orders its tiles by XCD (not part of the C ABI).  Plain C++ as well as HIP: the same functions
// run in the kernels' prologues and, compiled with g++, in tests/conv_rows/test_rows_cpu.py, which owns this arithmetic --
// the closed-form tap mask against a loop, the row walk against divmod, the remaps as bijections.
#pragma once
#include <stdint.h>
#include "loans_hip.h"
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define CONV_ROWS_FN __host__ __device__ __forceinline__
#else
#define CONV_ROWS_FN inline
#endif

// XCD-aware, bijective block remap: blocks that share an XCD (id % 8) get a contiguous range of tiles
CONV_ROWS_FN int xcd_remap(int id, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, xcd = id & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
}

// the weight-gradient halo kernels' remap (the channel-tile pairs that share a pixel range then share an L2): the same order
// when nblk is a multiple of 8, but the identity (no remap) otherwise
CONV_ROWS_FN int xcd_remap_whole(int id, int nblk) {
    const int per = nblk >> 3;
    if (per == 0 || (nblk & 7)) return id;
    return (id & 7) * per + (id >> 3);
}

// nx > 0: the taps are a row-major ny x nx grid, dy = dy0 + row * sdy, dx = dx0 + col * sdx, sd* = +-1
struct TapGrid {
    int nx, ny, dy0, sdy, dx0, sdx;
    unsigned long long rowpat;      // bit (row * nx) set for every row
};

// recognise such a grid (every convolution of this path has one); nx = 0 otherwise, and for one row of 64 taps, whose
// closed-form mask would shift by 64: tap_mask() then walks the tap list
inline TapGrid detect_tap_grid(const loans_igemm_desc* d) {
    TapGrid g = {0, 0, 0, 1, 0, 1, 0ull};
    int nx = 1;
    while (nx < d->ntaps && d->dy[nx] == d->dy[0]) ++nx;
    if (d->ntaps % nx || nx >= 64) return g;
    const int ny = d->ntaps / nx;
    const int sdx = nx > 1 ? d->dx[1] - d->dx[0] : 1;
    const int sdy = ny > 1 ? d->dy[nx] - d->dy[0] : 1;
    if ((sdx != 1 && sdx != -1) || (sdy != 1 && sdy != -1)) return g;
    for (int t = 0; t < d->ntaps; ++t)
        if (d->dy[t] != d->dy[0] + (t / nx) * sdy || d->dx[t] != d->dx[0] + (t % nx) * sdx) return g;
    g.nx = nx; g.ny = ny; g.dy0 = d->dy[0]; g.sdy = sdy; g.dx0 = d->dx[0]; g.sdx = sdx;
    for (int r = 0; r < ny; ++r) g.rowpat |= 1ull << (r * nx);
    return g;
}

CONV_ROWS_FN int rows_min(int a, int b) { return a < b ? a : b; }
CONV_ROWS_FN int rows_max(int a, int b) { return a > b ? a : b; }

// Bit t SET when tap t of the row whose base pixel is (iy0, ix0) reads inside the inH x inW image.  On a tap grid the
// in-bounds taps are an index RANGE per axis and the mask is two shifts and a multiply -- no loops, no table reads.
CONV_ROWS_FN unsigned long long tap_mask(const TapGrid& g, bool dense, int iy0, int ix0, int inH, int inW, int ntaps,
                                         const int8_t* dy, const int8_t* dx) {
    if (dense) return ~0ull;            // LOANS_F_DENSE: the caller's zero padding makes every tap readable
    unsigned long long mask = 0;
    if (g.nx > 0) {
        // column j valid <=> 0 <= ix0 + dx0 + j*sdx < inW  (sdx = +-1): a contiguous j range
        const int cx = ix0 + g.dx0, cy = iy0 + g.dy0;
        int jlo, jhi, rlo, rhi;
        if (g.sdx > 0) { jlo = rows_max(0, -cx); jhi = rows_min(g.nx, inW - cx); }
        else { jlo = rows_max(0, cx - inW + 1); jhi = rows_min(g.nx, cx + 1); }
        if (g.sdy > 0) { rlo = rows_max(0, -cy); rhi = rows_min(g.ny, inH - cy); }
        else { rlo = rows_max(0, cy - inH + 1); rhi = rows_min(g.ny, cy + 1); }
        if (jhi > jlo && rhi > rlo) {
            const unsigned long long colbits = ((1ull << jhi) - 1ull) & ~((1ull << jlo) - 1ull);     // jhi <= nx < 64
            const int blo = rlo * g.nx, bhi = rhi * g.nx;     // bhi <= 64
            const unsigned long long below_hi = bhi >= 64 ? ~0ull : ((1ull << bhi) - 1ull);
            const unsigned long long rowsel = g.rowpat & below_hi & ~((1ull << blo) - 1ull);
            mask = colbits * rowsel;       // colbits < 2^nx, rowsel bits nx apart: no carries
        }
    } else {
        for (int t = 0; t < ntaps; ++t) {
            const int iy = iy0 + dy[t], ix = ix0 + dx[t];
            if ((unsigned)iy < (unsigned)inH && (unsigned)ix < (unsigned)inW) mask |= 1ull << t;
        }
    }
    return mask;
}

// (image, grid row, grid column) of a GEMM row: two divisions for the first one, then steps of a few pixels
struct RowWalker {
    int b, y, x, gridH, gridW;
    float inv_gh, inv_gw;
    CONV_ROWS_FN RowWalker(int m0, int gridH_, int gridW_)
        : gridH(gridH_), gridW(gridW_), inv_gh(1.f / (float)gridH_), inv_gw(1.f / (float)gridW_) {
        const int gHW = gridH * gridW;
        b = m0 / gHW;
        const int rem = m0 - b * gHW;
        y = rem / gridW;
        x = rem - y * gridW;
    }
    // `step` rows on: exact floor((v + .5) / n) for the small integers involved
    CONV_ROWS_FN void advance(int step) {
        x += step;
        const int qx = (int)(((float)x + 0.5f) * inv_gw);
        x -= qx * gridW;
        y += qx;
        const int qy = (int)(((float)y + 0.5f) * inv_gh);
        y -= qy * gridH;
        b += qy;
    }
};

// what the kernels' launches differ in, as one thread of the prologue sees it
struct RowLaunch {
    int m0, M;                      // this thread's first GEMM row; rows end at M
    int gridH, gridW, oy0, ox0;     // the pixel grid the rows enumerate and its phase in the output (per class in a class launch)
    int ntaps;
    const int8_t* dy;               // the tap list (per class), read where the taps are no grid
    const int8_t* dx;
    unsigned out_pixel_bytes;       // output channels x bytes per output element
    unsigned in_unit_bytes;         // bytes per unit of inW / ix: a gathered pixel, or with LOANS_F_DENSE (inW / isx / dx count
    bool dense;                     // elements of packed rows) one element; dense: no tap is ever masked
};

// Per row (fixed for the whole K loop) of the RA rows a thread stages, STEP rows apart: rowoff = byte offset of its base
// pixel in the gathered tensor, badmask = bit t SET when tap t must read zero (outside the image, or the row does not
// exist), and -- from the thread with `store_opix` among those that share the row -- opix[STEP * i] = byte offset of its
// output pixel, ~0u = no row.
template <int RA, int STEP, typename MaskT>
CONV_ROWS_FN void row_prologue(const loans_igemm_desc& d, const TapGrid g, const RowLaunch l,
                               unsigned (&rowoff)[RA], MaskT (&badmask)[RA], unsigned* opix, bool store_opix) {
    // (everything read from the descriptor is read here, once: behind the stores to opix the compiler reads it again)
    const int inH = d.inH, inW = d.inW, isy = d.isy, isx = d.isx, outH = d.outH, outW = d.outW, osy = d.osy, osx = d.osx;
    RowWalker w(l.m0, l.gridH, l.gridW);
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int i = 0; i < RA; ++i) {
        unsigned pixoff = 0xFFFFFFFFu;
        unsigned long long mask = 0;
        rowoff[i] = 0;
        if (l.m0 + STEP * i < l.M) {
            const int iy0 = w.y * isy, ix0 = w.x * isx;
            rowoff[i] = (unsigned)((w.b * inH + iy0) * inW + ix0) * l.in_unit_bytes;
            pixoff = (unsigned)((w.b * outH + w.y * osy + l.oy0) * outW + w.x * osx + l.ox0) * l.out_pixel_bytes;
            mask = tap_mask(g, l.dense, iy0, ix0, inH, inW, l.ntaps, l.dy, l.dx);
        }
        badmask[i] = (MaskT)~mask;
        if (store_opix) opix[STEP * i] = pixoff;
        w.advance(STEP);
    }
}

// ---- image-strided row tiles (LOANS_TILE_POSMAJOR) ----------------------------------------------------------------------------
// A row tile holds ONE grid position of BM consecutive images: rows pos + (ig * BM + j) * gridH * gridW of the ordinary GEMM row
// space, j = 0 .. BM - 1.  The tap mask then is the same for every row of the block, and the block's K loop leaves out the taps
// that read outside the frame.  tests/conv_posmajor/test_rows_cpu.py owns this arithmetic.

// row tile -> (image group, grid position): the position is the fast index, so that the tiles next to each other (one XCD's, after
// the remap) gather neighbouring -- overlapping -- input pixels of the same images
CONV_ROWS_FN void images_tile(int tile_m, int npos, int* ig, int* pos) {
    *ig = tile_m / npos;
    *pos = tile_m - *ig * npos;
}
CONV_ROWS_FN int images_tiles(int B, int gridH, int gridW, int BM) { return gridH * gridW * ((B + BM - 1) / BM); }

// the taps a block at grid position `pos` runs: bit t SET when tap t reads inside the frame there, and how many are.  From
// block-uniform values only.  A position with no tap inside (1 x 1 / pad 1 at the rim) keeps tap 0 -- its lanes are masked and read
// zeros -- so that no block runs an empty K loop.
struct BlockTaps {
    unsigned long long mask;
    int count;
};
CONV_ROWS_FN BlockTaps block_taps(const loans_igemm_desc& d, const TapGrid& g, int gridW, int pos, int ntaps, const int8_t* dy,
                                  const int8_t* dx) {
    const int y = pos / gridW, x = pos - y * gridW;
    unsigned long long m = tap_mask(g, false, y * d.isy, x * d.isx, d.inH, d.inW, ntaps, dy, dx);
    if (!m) m = 1ull;
    return {m, __builtin_popcountll(m)};
}

// The per-tap loader's walk along K over the taps of `mask` only, `cpc` 32-deep chunks per tap: the tap and the chunk within it of
// the chunk loaded next, the scalar byte offsets into the tap's channels (sof_a) and along a weight row (sof_b; rows keep ALL taps).
struct TapWalk {
    unsigned long long left;        // the taps not yet finished, the current one included
    int ktap, kcw;
    unsigned sof_a, sof_b;
};
CONV_ROWS_FN void tap_walk_begin(TapWalk& w, unsigned long long mask, int cpc) {
    w.left = mask;
    w.ktap = __builtin_ctzll(mask);         // (mask != 0: block_taps)
    w.kcw = 0;
    w.sof_a = 0u;
    w.sof_b = 128u * (unsigned)(w.ktap * cpc);
}
// one chunk on; true when that chunk starts another tap (behind the last tap the state stays on it: nothing is loaded from there)
CONV_ROWS_FN bool tap_walk_next(TapWalk& w, int cpc) {
    w.sof_a += 128u;
    w.sof_b += 128u;
    if (++w.kcw != cpc) return false;
    w.kcw = 0;
    w.sof_a = 0u;
    w.left &= w.left - 1ull;
    if (w.left) {
        w.ktap = __builtin_ctzll(w.left);
        w.sof_b = 128u * (unsigned)(w.ktap * cpc);
    }
    return true;
}

// row_prologue for such a tile: l.m0 = this thread's first IMAGE (ig * BM + its row of the tile), l.M = the image count; row i is
// image l.m0 + STEP * i at grid position `pos` and exists iff that image does.  Same rowoff / opix / badmask as row_prologue().
template <int RA, int STEP, typename MaskT>
CONV_ROWS_FN void row_prologue_images(const loans_igemm_desc& d, const TapGrid g, const RowLaunch l, int pos,
                                      unsigned (&rowoff)[RA], MaskT (&badmask)[RA], unsigned* opix, bool store_opix) {
    const int inH = d.inH, inW = d.inW, isy = d.isy, isx = d.isx, outH = d.outH, outW = d.outW, osy = d.osy, osx = d.osx;
    const int y = pos / l.gridW, x = pos - y * l.gridW;
    const int iy0 = y * isy, ix0 = x * isx;
    const unsigned long long mask = tap_mask(g, l.dense, iy0, ix0, inH, inW, l.ntaps, l.dy, l.dx);
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int i = 0; i < RA; ++i) {
        const int b = l.m0 + STEP * i;
        const bool exists = b < l.M;
        rowoff[i] = exists ? (unsigned)((b * inH + iy0) * inW + ix0) * l.in_unit_bytes : 0u;
        badmask[i] = (MaskT)~(exists ? mask : 0ull);
        if (store_opix)
            opix[STEP * i] = exists ? (unsigned)((b * outH + y * osy + l.oy0) * outW + x * osx + l.ox0) * l.out_pixel_bytes : 0xFFFFFFFFu;
    }
}
