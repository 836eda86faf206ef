// Stand-alone check of the image-strided row tiles of loans_amd/csrc/conv_rows.h (LOANS_TILE_POSMAJOR) as plain C++
// (tests/conv_posmajor/test_rows_cpu.py compiles it with -fsanitize=address,undefined and runs it): the prologue against a
// brute-force loop over the ordinary GEMM rows, the tiles as an exact cover of those rows, the block's tap set against the AND
// of its rows' masks, the compacted K walk against the full walk with the left-out taps filtered away.  One line per check;
// exit status 0 = pass.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "conv_rows.h"

static long long g_checks = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        ++g_checks;                                             \
        if (!(cond)) {                                          \
            std::printf("FAILED %s:%d: ", __FILE__, __LINE__);  \
            std::printf(__VA_ARGS__);                           \
            std::printf("\n");                                  \
            std::exit(1);                                       \
        }                                                       \
    } while (0)

// the tap lists and geometries the launches of this path come with (loans_amd/ops.py, ConvGeometry)
struct Geom {
    const char* name;
    int k, stride, pad;
    bool dgrad;         // the stride-parity class (0, 0) of the data gradient: taps descend
};
static const Geom GEOMS[] = {
    {"3x3/1 forward", 3, 1, 1, false}, {"3x3/1 data gradient", 3, 1, 1, true}, {"4x4/2 forward", 4, 2, 1, false},
    {"4x4/2 data gradient", 4, 2, 1, true}, {"1x1/1 pad 0", 1, 1, 0, false}, {"1x1/1 pad 1", 1, 1, 1, false},
    {"3x3/2 forward", 3, 2, 1, false}, {"3x3/2 data gradient", 3, 2, 1, true},
};

// descriptor for a gridH x gridW grid of rows: forward = the output frame of a k / stride / pad convolution whose input is the
// largest that gives it; data gradient = class (0, 0), gathered tensor gridH x gridW, output (the forward input) stride apart
static loans_igemm_desc make_desc(const Geom& q, int B, int gridH, int gridW, int Cin, int Cout) {
    loans_igemm_desc d;
    std::memset(&d, 0, sizeof d);
    d.B = B; d.Cin = Cin; d.Cout = Cout; d.gridH = gridH; d.gridW = gridW;
    if (!q.dgrad) {
        d.inH = (gridH - 1) * q.stride + q.k - 2 * q.pad; d.inW = (gridW - 1) * q.stride + q.k - 2 * q.pad;
        if (d.inH < 1) d.inH = 1;
        if (d.inW < 1) d.inW = 1;
        d.outH = gridH; d.outW = gridW; d.osy = d.osx = 1; d.isy = d.isx = q.stride;
        for (int r = 0; r < q.k; ++r)
            for (int s = 0; s < q.k; ++s) { d.dy[d.ntaps] = (int8_t)(r - q.pad); d.dx[d.ntaps] = (int8_t)(s - q.pad); ++d.ntaps; }
    } else {
        d.inH = gridH; d.inW = gridW;           // gy; the class's grid is taken as large as gy here
        d.outH = gridH * q.stride; d.outW = gridW * q.stride; d.osy = d.osx = q.stride; d.isy = d.isx = 1;
        for (int r = 0; r < q.k; ++r) {
            if ((q.pad - r) % q.stride) continue;
            for (int s = 0; s < q.k; ++s) {
                if ((q.pad - s) % q.stride) continue;
                d.dy[d.ntaps] = (int8_t)((q.pad - r) / q.stride); d.dx[d.ntaps] = (int8_t)((q.pad - s) / q.stride); ++d.ntaps;
            }
        }
    }
    return d;
}

struct Row { unsigned rowoff, opix; unsigned long long bad; };

// the definition: GEMM row m = (b, y, x) of the ordinary row space, straight from loans_hip.h
static Row brute_row(const loans_igemm_desc& d, int m, unsigned in_unit, unsigned out_pixel) {
    const int gHW = d.gridH * d.gridW, b = m / gHW, y = m % gHW / d.gridW, x = m % d.gridW;
    Row r;
    r.rowoff = (unsigned)((b * d.inH + y * d.isy) * d.inW + x * d.isx) * in_unit;
    r.opix = (unsigned)((b * d.outH + y * d.osy + d.oy0) * d.outW + x * d.osx + d.ox0) * out_pixel;
    unsigned long long ok = 0;
    for (int t = 0; t < d.ntaps; ++t) {
        const int iy = y * d.isy + d.dy[t], ix = x * d.isx + d.dx[t];
        if (iy >= 0 && iy < d.inH && ix >= 0 && ix < d.inW) ok |= 1ull << t;
    }
    r.bad = ~ok;
    return r;
}

template <int BM>
static void check_geometry(const Geom& q, int gridH, int gridW, int B, long long* rows_seen, long long* empty_blocks) {
    constexpr int RA = BM / 32;
    const int Cin = 32, Cout = 8;
    const loans_igemm_desc d = make_desc(q, B, gridH, gridW, Cin, Cout);
    const TapGrid g = detect_tap_grid(&d);
    CHECK(g.nx > 0, "%s: taps on a grid", q.name);
    const unsigned in_unit = (unsigned)Cin * 4u, out_pixel = (unsigned)Cout * 4u;
    const int npos = gridH * gridW, M = B * npos, tiles = images_tiles(B, gridH, gridW, BM);
    CHECK(tiles == npos * ((B + BM - 1) / BM), "tile count");
    std::vector<int> covered(M, 0);
    std::vector<unsigned> opix(BM);
    for (int tm = 0; tm < tiles; ++tm) {
        int ig, pos;
        images_tile(tm, npos, &ig, &pos);
        CHECK(ig >= 0 && ig * BM < B && pos >= 0 && pos < npos && ig * npos + pos == tm, "tile %d -> (%d, %d)", tm, ig, pos);
        if (tm + 1 < tiles && pos + 1 < npos) {      // the position is the fast index
            int ig2, pos2;
            images_tile(tm + 1, npos, &ig2, &pos2);
            CHECK(ig2 == ig && pos2 == pos + 1, "neighbouring tiles are neighbouring positions");
        }
        std::fill(opix.begin(), opix.end(), 0x12345678u);
        unsigned long long all_ok = ~0ull;
        int real_rows = 0;
        for (int lrow = 0; lrow < 32; ++lrow) {         // the threads of a block, as the kernel calls it
            unsigned rowoff[RA];
            unsigned long long bad[RA];
            const RowLaunch l = {ig * BM + lrow, B, gridH, gridW, d.oy0, d.ox0, d.ntaps, d.dy, d.dx, out_pixel, in_unit, false};
            row_prologue_images<RA, 32>(d, g, l, pos, rowoff, bad, opix.data() + lrow, true);
            for (int i = 0; i < RA; ++i) {
                const int img = ig * BM + lrow + 32 * i;
                if (img < B) {
                    const int m = pos + img * npos;
                    const Row want = brute_row(d, m, in_unit, out_pixel);
                    CHECK(rowoff[i] == want.rowoff && bad[i] == want.bad && opix[lrow + 32 * i] == want.opix,
                          "%s grid %d x %d B %d tile %d row %d: off %u/%u opix %u/%u bad %llx/%llx", q.name, gridH, gridW, B, tm, lrow + 32 * i,
                          rowoff[i], want.rowoff, opix[lrow + 32 * i], want.opix, bad[i], want.bad);
                    ++covered[m];
                    all_ok &= ~bad[i];
                    ++real_rows;
                    ++*rows_seen;
                } else {
                    CHECK(bad[i] == ~0ull && opix[lrow + 32 * i] == 0xFFFFFFFFu && rowoff[i] == 0u, "a row without an image is masked");
                }
            }
        }
        CHECK(real_rows >= 1, "no tile without a row");
        // the block's taps: the AND of its rows' masks (they are all the same), tap 0 where that is empty
        const BlockTaps bt = block_taps(d, g, gridW, pos, d.ntaps, d.dy, d.dx);
        const unsigned long long in_range = d.ntaps < 64 ? (1ull << d.ntaps) - 1ull : ~0ull;
        unsigned long long want_mask = all_ok & in_range;
        if (!want_mask) { want_mask = 1ull; ++*empty_blocks; }
        CHECK(bt.mask == want_mask && bt.count == __builtin_popcountll(want_mask) && bt.count >= 1 && bt.count <= d.ntaps,
              "%s grid %d x %d pos %d: taps %llx (%d), want %llx", q.name, gridH, gridW, pos, bt.mask, bt.count, want_mask);
        // the compacted walk == the full walk of the per-tap loader without the chunks of the taps left out
        for (int cpc = 1; cpc <= 3; ++cpc) {
            TapWalk w;
            tap_walk_begin(w, bt.mask, cpc);
            int n = 0;
            for (int c = 0; c < d.ntaps * cpc; ++c) {       // full walk: chunk c = (tap c / cpc, chunk c % cpc), weights at 128 * c
                const int tap = c / cpc, kcw = c % cpc;
                if (!((bt.mask >> tap) & 1)) continue;
                CHECK(w.ktap == tap && w.kcw == kcw && w.sof_a == 128u * (unsigned)kcw && w.sof_b == 128u * (unsigned)c,
                      "walk chunk %d of mask %llx cpc %d: tap %d/%d kcw %d/%d sof_a %u sof_b %u/%u", n, bt.mask, cpc, w.ktap, tap, w.kcw, kcw,
                      w.sof_a, w.sof_b, 128u * (unsigned)c);
                const bool new_tap = tap_walk_next(w, cpc);
                CHECK(new_tap == (kcw == cpc - 1), "the tap-change flag");
                ++n;
            }
            CHECK(n == bt.count * cpc && w.left == 0ull, "the walk has popcount x cpc chunks");
        }
    }
    for (int m = 0; m < M; ++m) CHECK(covered[m] == 1, "%s grid %d x %d B %d: row %d covered %d times", q.name, gridH, gridW, B, m, covered[m]);
}

int main() {
    for (const Geom& q : GEOMS) {
        long long rows = 0, empty = 0;
        for (int gridH = 1; gridH <= 9; ++gridH)
            for (int gridW = 1; gridW <= 9; ++gridW)
                for (int B = 1; B <= 2 * 64 + 1; B += (B < 4 || (B >= 62 && B < 66) || B >= 126) ? 1 : 7) {
                    check_geometry<64>(q, gridH, gridW, B, &rows, &empty);
                    if (B <= 2 * 32 + 1) check_geometry<32>(q, gridH, gridW, B, &rows, &empty);
                }
        std::printf("%s: %lld rows == brute force, each covered once; %lld blocks with no tap inside keep tap 0\n", q.name, rows, empty);
    }
    // an empty mask keeps exactly tap 0, whatever the tap list: 1 x 1 / pad 1 at the rim, 3 x 3 reading two pixels off the frame
    {
        const loans_igemm_desc d = make_desc(GEOMS[5], 64, 3, 3, 32, 8);
        const TapGrid g = detect_tap_grid(&d);
        int empties = 0;
        for (int pos = 0; pos < 9; ++pos) {
            const BlockTaps bt = block_taps(d, g, 3, pos, d.ntaps, d.dy, d.dx);
            CHECK(bt.mask == 1ull && bt.count == 1, "1 x 1 taps");
            unsigned rowoff[2];
            unsigned long long bad[2];
            unsigned opix[64];
            const RowLaunch l = {0, 64, 3, 3, 0, 0, 1, d.dy, d.dx, 32u, 128u, false};
            row_prologue_images<2, 32>(d, g, l, pos, rowoff, bad, opix, true);
            empties += (bad[0] & 1ull) != 0;        // the kept tap is masked in every row: the block reads zeros
        }
        CHECK(empties == 8, "eight of nine positions of a 1 x 1 / pad 1 frame of one pixel have no tap inside: %d", empties);
        std::printf("empty masks keep tap 0, masked in every row\n");
    }
    std::printf("ok: %lld checks\n", g_checks);
    return 0;
}
