// Stand-alone check of loans_amd/csrc/conv_rows.h as plain C++ (tests/conv_rows/test_rows_cpu.py compiles it with
// -fsanitize=address,undefined and runs it): the closed-form tap mask against a brute-force one, the tap-grid detector,
// the row walk against integer division, the block remaps as bijections.  Prints one line per check; exit status 0 = pass.
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

// the definition: tap t reads pixel (iy0 + dy[t], ix0 + dx[t]); bit t is set when that pixel exists
static unsigned long long brute_mask(int ntaps, const int8_t* dy, const int8_t* dx, int iy0, int ix0, int inH, int inW) {
    unsigned long long m = 0;
    for (int t = 0; t < ntaps; ++t) {
        const int iy = iy0 + dy[t], ix = ix0 + dx[t];
        if (iy >= 0 && iy < inH && ix >= 0 && ix < inW) m |= 1ull << t;
    }
    return m;
}

static loans_igemm_desc grid_desc(int ny, int nx, int dy0, int sdy, int dx0, int sdx) {
    loans_igemm_desc d;
    std::memset(&d, 0, sizeof d);
    d.ntaps = ny * nx;
    for (int r = 0; r < ny; ++r)
        for (int j = 0; j < nx; ++j) {
            d.dy[r * nx + j] = (int8_t)(dy0 + r * sdy);
            d.dx[r * nx + j] = (int8_t)(dx0 + j * sdx);
        }
    return d;
}

// one axis of a row's situation: first tap offset, image size, base coordinate
struct Axis { int d0, size, i0; };

static std::vector<Axis> axis_cases() {
    std::vector<Axis> v;
    for (int d0 = -7; d0 <= 7; ++d0)
        for (int size = 1; size <= 9; ++size)
            for (int i0 = -10; i0 <= size + 10; ++i0) v.push_back({d0, size, i0});
    return v;
}

// Closed form == brute force.  Every grid shape 1..8 x 1..8 (16, 49 and 64 taps among them: bhi == 64) with either sign per
// axis, and per axis every (d0, size, i0) of axis_cases().  The whole product has 3e9 rows; the mask is a product of an x part
// and a y part, so the full set of one axis is crossed with a stride through the other axis's set, whose phase moves with the
// first axis's index and the grid shape -- and then the other way round.
static void check_tap_mask() {
    const std::vector<Axis> ax = axis_cases();
    const int n = (int)ax.size(), stride = 421;         // 3510 cases per axis; 421 is prime
    const TapGrid none = {0, 0, 0, 1, 0, 1, 0ull};
    std::vector<loans_igemm_desc> descs(15 * 15);
    std::vector<TapGrid> grids(15 * 15);
    long long calls = 0;
    for (int ny = 1; ny <= 8; ++ny)
        for (int nx = 1; nx <= 8; ++nx)
            for (int sdy = -1; sdy <= 1; sdy += 2)
                for (int sdx = -1; sdx <= 1; sdx += 2) {
                    for (int dy0 = -7; dy0 <= 7; ++dy0)
                        for (int dx0 = -7; dx0 <= 7; ++dx0) {
                            const int e = (dy0 + 7) * 15 + dx0 + 7;
                            descs[e] = grid_desc(ny, nx, dy0, sdy, dx0, sdx);
                            grids[e] = detect_tap_grid(&descs[e]);
                            CHECK(grids[e].nx == nx && grids[e].ny == ny && grids[e].dy0 == dy0 && grids[e].dx0 == dx0 &&
                                  grids[e].sdy == (ny > 1 ? sdy : 1) && grids[e].sdx == (nx > 1 ? sdx : 1),
                                  "grid %d x %d detected as %d x %d", ny, nx, grids[e].ny, grids[e].nx);
                        }
                    for (int pass = 0; pass < 2; ++pass)
                        for (int i = 0; i < n; ++i)
                            for (int k = (i * 7 + ny * 8 + nx) % stride; k < n; k += stride) {
                                const Axis& X = pass ? ax[k] : ax[i];
                                const Axis& Y = pass ? ax[i] : ax[k];
                                const loans_igemm_desc& d = descs[(Y.d0 + 7) * 15 + X.d0 + 7];
                                const TapGrid& g = grids[(Y.d0 + 7) * 15 + X.d0 + 7];
                                const unsigned long long want = brute_mask(d.ntaps, d.dy, d.dx, Y.i0, X.i0, Y.size, X.size);
                                const unsigned long long got = tap_mask(g, false, Y.i0, X.i0, Y.size, X.size, d.ntaps, d.dy, d.dx);
                                CHECK(got == want, "grid %d x %d sd %d %d d0 %d %d in %d x %d at %d %d: %llx, want %llx", ny, nx, sdy, sdx,
                                      Y.d0, X.d0, Y.size, X.size, Y.i0, X.i0, got, want);
                                if ((calls++ & 15) == 0) {      // the loop fallback on the same row, and the dense shortcut
                                    CHECK(tap_mask(none, false, Y.i0, X.i0, Y.size, X.size, d.ntaps, d.dy, d.dx) == want, "loop fallback");
                                    CHECK(tap_mask(g, true, Y.i0, X.i0, Y.size, X.size, d.ntaps, d.dy, d.dx) == ~0ull, "dense");
                                }
                            }
                }
    std::printf("tap_mask: %lld rows, closed form == brute force\n", calls);

    // a tap list that is no grid (a plus sign) takes the loop
    loans_igemm_desc d;
    std::memset(&d, 0, sizeof d);
    const int8_t pdy[5] = {-1, 0, 0, 0, 1}, pdx[5] = {0, -1, 0, 1, 0};
    d.ntaps = 5;
    std::memcpy(d.dy, pdy, 5);
    std::memcpy(d.dx, pdx, 5);
    const TapGrid g = detect_tap_grid(&d);
    CHECK(g.nx == 0, "a plus sign is no grid");
    for (int inH = 1; inH <= 4; ++inH)
        for (int inW = 1; inW <= 4; ++inW)
            for (int iy0 = -3; iy0 <= inH + 2; ++iy0)
                for (int ix0 = -3; ix0 <= inW + 2; ++ix0)
                    CHECK(tap_mask(g, false, iy0, ix0, inH, inW, 5, d.dy, d.dx) == brute_mask(5, d.dy, d.dx, iy0, ix0, inH, inW), "plus sign");
    std::printf("tap_mask: non-grid tap list == brute force\n");
}

// forward taps of a k x k kernel with padding p; the taps of the stride-parity class (py, px) of its stride-s data gradient
// as loans_amd/ops.py (ConvGeometry) lists them: the kernel positions (ky, kx) with py + p - ky and px + p - kx multiples of
// s, row-major in ascending order -- so dy = (py + p - ky) / s and dx DEScend: a grid with sdy = sdx = -1
static loans_igemm_desc fwd_desc(int k, int p) { return grid_desc(k, k, -p, 1, -p, 1); }

static loans_igemm_desc dgrad_class_desc(int k, int s, int p, int py, int px) {
    loans_igemm_desc d;
    std::memset(&d, 0, sizeof d);
    for (int ky = 0; ky < k; ++ky) {
        if ((py + p - ky) % s) continue;
        for (int kx = 0; kx < k; ++kx) {
            if ((px + p - kx) % s) continue;
            d.dy[d.ntaps] = (int8_t)((py + p - ky) / s);
            d.dx[d.ntaps] = (int8_t)((px + p - kx) / s);
            ++d.ntaps;
        }
    }
    return d;
}

static void check_detect() {
    const int ks[4] = {1, 3, 4, 7};
    for (int k : ks) {
        const loans_igemm_desc d = fwd_desc(k, k / 2);
        const TapGrid g = detect_tap_grid(&d);
        CHECK(g.nx == k && g.ny == k && g.dy0 == -(k / 2) && g.dx0 == -(k / 2) && g.sdy == 1 && g.sdx == 1, "forward %d x %d", k, k);
        unsigned long long pat = 0;
        for (int r = 0; r < k; ++r) pat |= 1ull << (r * k);
        CHECK(g.rowpat == pat, "forward %d x %d row pattern", k, k);
    }
    // 3 x 3 / 2, pad 1: classes of 1, 2, 2 and 4 taps; 4 x 4 / 2, pad 1: four classes of 2 x 2 taps
    int taps3[4], n3 = 0;
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px) {
            const loans_igemm_desc d3 = dgrad_class_desc(3, 2, 1, py, px);
            const TapGrid g3 = detect_tap_grid(&d3);
            CHECK(g3.nx > 0 && g3.nx * g3.ny == d3.ntaps && (g3.ny == 1 || g3.sdy == -1) && (g3.nx == 1 || g3.sdx == -1), "3x3/2 class (%d, %d): %d taps seen as %d x %d", py, px, d3.ntaps, g3.ny, g3.nx);
            taps3[n3++] = d3.ntaps;
            const loans_igemm_desc d4 = dgrad_class_desc(4, 2, 1, py, px);
            const TapGrid g4 = detect_tap_grid(&d4);
            CHECK(d4.ntaps == 4 && g4.nx == 2 && g4.ny == 2 && g4.sdy == -1 && g4.sdx == -1, "4x4/2 class (%d, %d): %d taps seen as %d x %d", py, px, d4.ntaps, g4.ny, g4.nx);
            for (const loans_igemm_desc* d : {&d3, &d4}) {      // and the mask of such a class, on a small image
                const TapGrid g = detect_tap_grid(d);
                for (int iy0 = -2; iy0 <= 6; ++iy0)
                    for (int ix0 = -2; ix0 <= 6; ++ix0)
                        CHECK(tap_mask(g, false, iy0, ix0, 5, 5, d->ntaps, d->dy, d->dx) == brute_mask(d->ntaps, d->dy, d->dx, iy0, ix0, 5, 5),
                              "class mask");
            }
        }
    CHECK(taps3[0] + taps3[1] + taps3[2] + taps3[3] == 9 && taps3[0] * taps3[1] * taps3[2] * taps3[3] == 16, "3x3/2 classes: 1, 2, 2, 4 taps");
    // declined: a hole, a step of 2, one row of 64 taps
    loans_igemm_desc d = fwd_desc(3, 1);
    d.dx[4] = 5;
    CHECK(detect_tap_grid(&d).nx == 0, "a list with a hole");
    d = grid_desc(3, 3, -2, 2, -1, 1);
    CHECK(detect_tap_grid(&d).nx == 0, "rows 2 apart");
    d = grid_desc(1, 3, 0, 1, -2, 1);
    d.dx[1] = 0; d.dx[2] = 2;
    CHECK(detect_tap_grid(&d).nx == 0, "columns 2 apart");
    d = grid_desc(1, 64, 0, 1, -32, 1);
    const TapGrid g64 = detect_tap_grid(&d);
    CHECK(g64.nx == 0, "1 x 64 taps");
    for (int ix0 = -40; ix0 <= 50; ++ix0)
        CHECK(tap_mask(g64, false, 0, ix0, 1, 9, 64, d.dy, d.dx) == brute_mask(64, d.dy, d.dx, 0, ix0, 1, 9), "1 x 64 mask");
    d = grid_desc(2, 32, 0, 1, -16, 1);
    CHECK(detect_tap_grid(&d).nx == 32, "2 x 32 taps");
    std::printf("detect_tap_grid: forward 1/3/4/7, data-gradient classes, three refusals\n");
}

// every grid 1..300 x 1..300 with both row steps; start rows 0 .. 3 gridH gridW (three images): all of them on small grids,
// about sixty evenly spread ones on large grids; each walked 8 steps
static void check_walker() {
    const int steps[2] = {32, 64};
    long long n = 0;
    for (int gridW = 1; gridW <= 300; ++gridW)
        for (int gridH = 1; gridH <= 300; ++gridH)
            for (int step : steps) {
                const int gHW = gridH * gridW, stride = 3 * gHW / 61 + 1;
                for (int m0 = 0; m0 <= 3 * gHW; m0 += stride) {
                    RowWalker w(m0, gridH, gridW);
                    for (int i = 0; i <= 8; ++i) {
                        const int m = m0 + i * step;
                        CHECK(w.b == m / gHW && w.y == m % gHW / gridW && w.x == m % gridW, "grid %d x %d row %d + %d x %d: (%d, %d, %d)", gridH,
                              gridW, m0, i, step, w.b, w.y, w.x);
                        w.advance(step);
                        ++n;
                    }
                }
            }
    std::printf("RowWalker: %lld steps == divmod\n", n);
}

static void check_remap() {
    std::vector<char> seen;
    for (int nblk = 1; nblk <= 4096; ++nblk)
        for (int which = 0; which < 2; ++which) {
            seen.assign(nblk, 0);
            for (int id = 0; id < nblk; ++id) {
                const int l = which ? xcd_remap_whole(id, nblk) : xcd_remap(id, nblk);
                CHECK(l >= 0 && l < nblk && !seen[l], "remap %d of %d blocks: %d -> %d", which, nblk, id, l);
                seen[l] = 1;
                if (which && (nblk & 7)) CHECK(l == id, "the halo remap is the identity for %d blocks", nblk);
                if (which && !(nblk & 7)) CHECK(l == xcd_remap(id, nblk), "the two remaps agree on %d blocks", nblk);
            }
        }
    std::printf("xcd_remap, xcd_remap_whole: bijections of 0 .. nblk - 1 for nblk = 1 .. 4096\n");
}

int main() {
    check_detect();
    check_tap_mask();
    check_walker();
    check_remap();
    std::printf("ok: %lld checks\n", g_checks);
    return 0;
}
