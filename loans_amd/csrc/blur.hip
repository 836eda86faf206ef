// Anti-aliased downsampling (Zhang 2019, "Making Convolutional Networks Shift-Invariant Again"; functions/blocks.py, blur=True):
//     blur(a)[b,i,j,c] = 1/16 sum_{di,dj in 0..2} w[di] w[dj] a[b, refl(2i + di - 1), refl(2j + dj - 1), c],   w = (1, 2, 1),
// reflect padding of one (refl(-1) = 1, refl(H) = H - 2), ceil(H / 2) x ceil(W / 2) outputs, on NHWC tensors in fp32 or bf16
// storage.  A strided stage of a residual unit runs its convolution at stride 1 and hands blur(relu(bn(conv))) on; neither the
// full-resolution activation nor its gradient exists:
//   forward ........ y = blur(act(scale x + shift)) in one pass; without coefficients the plain blur(x) of the shortcut
//   reduction ...... gz = blurT(gy) (scale x + shift > 0) formed on the fly; sum gz and sum gz (x - mean) per channel
//   apply .......... gx = k1 gz + k2 x + k3, gz by the same device function: the bits whose sums were taken
//   plain .......... gx = blurT(gy) [+ addend]: the shortcut arm joins the main branch's gradient
//
// How the work is split.  A thread owns a 16-byte channel unit (4 fp32 / 8 bf16 channels), a block a tile of BL_TH x BL_TW
// positions of the QUARTER-resolution map of one sample for a chunk of 64 channels, and walks the chunks blockIdx.z, + gridDim.z,
// ...  The forward stages the (2 BL_TH + 1) x (2 BL_TW + 1) input halo into LDS as fp32 -- BN and ReLU applied once per element
// on the way in, the reflected rows and columns resolved there -- and every output is a horizontal 1 2 1 of three LDS rows
// into registers, then the vertical one.  The backward passes stage the (BL_TH + 1) x (BL_TW + 1) halo of gy (zeros outside the
// map) and own the 2 BL_TH x 2 BL_TW full-resolution positions under the tile: the transposed stencil is a GATHER of at most
// 2 x 2 values of gy whose weights fold the reflected border into rows / columns 1 and H - 2 (blur_tap), so nothing is
// scattered.  Every product is by 0, 1, 2 or 1/16 and therefore exact; an output rounds twice (horizontal, vertical), in a fixed
// order.  The reduction leaves one fp64 record per block, [B x tiles][2][C]; a second small launch folds them in record order
// into replica 0 of the [replicas][2][C] accumulators loans_bn_bwd_coeffs_rep_f32 reads (centred = 1).  No floating-point
// atomics: two runs give the same bits.  Nothing waits for the host.
#include "common.h"
#include "unit16.h"

namespace {

constexpr int BL_TH = 4, BL_TW = 8;                              // quarter-resolution tile of a block: rows x columns
constexpr int BL_HH = 2 * BL_TH + 1, BL_HW = 2 * BL_TW + 1;      // forward: the input halo
constexpr int BL_GH = BL_TH + 1, BL_GW = BL_TW + 1;              // backward: the halo of gy
constexpr int BL_CH = 64;                                        // channels of a chunk: one LDS row per position
constexpr int BL_MAX_C = 2048, BL_MAX_Z = 8;

__device__ __forceinline__ f32x4 fma4(f32x4 a, f32x4 b, f32x4 c) {
    return f32x4{fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w)};
}
__device__ __forceinline__ f32x4 splat4(float v) { return f32x4{v, v, v, v}; }
// a + 2 b + c: the product is exact, the two additions round in this order
__device__ __forceinline__ f32x4 tap121(f32x4 a, f32x4 b, f32x4 c) { return fma4(splat4(2.f), b, a + c); }
__device__ __forceinline__ f32x4 lds4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// refl() for an index in -1 .. n (the only ones a tap of a valid output reaches)
__device__ __forceinline__ int blur_refl(int i, int n) { return i < 0 ? 1 : (i >= n ? n - 2 : i); }

// ---- forward ---------------------------------------------------------------------------------------------------------------------
template <bool AFF, typename T>
__global__ __launch_bounds__(256) void blur_fwd_kernel(const T* x, const float* scale, const float* shift, T* y, int H, int W, int Ho,
                                                       int Wo, int C, int tiles_w) {
    constexpr int V = unit16<T>::V, NV = unit16<T>::NV, CU = BL_CH / V, PP = 256 / CU;      // PP positions per pass of the block
    __shared__ __attribute__((aligned(16))) float tile[BL_HH * BL_HW][BL_CH];
    const int tid = threadIdx.x, u = tid % CU, p0 = tid / CU;
    const int i0 = (int)(blockIdx.x / tiles_w) * BL_TH, j0 = (int)(blockIdx.x % tiles_w) * BL_TW;
    x += (int64_t)blockIdx.y * H * W * C;
    y += (int64_t)blockIdx.y * Ho * Wo * C;
    for (int ch = blockIdx.z * BL_CH; ch < C; ch += gridDim.z * BL_CH) {
        const int c = ch + u * V;
        f32x4 s[NV], t[NV];
        if (AFF) {
#pragma unroll
            for (int q = 0; q < NV; ++q) { s[q] = ld4(scale + c + 4 * q); t[q] = ld4(shift + c + 4 * q); }
        }
#pragma unroll 5
        for (int p = p0; p < BL_HH * BL_HW; p += PP) {
            const int hr = p / BL_HW, hc = p - hr * BL_HW;
            const int r = 2 * i0 + hr - 1, cc = 2 * j0 + hc - 1;
            if (r > H || cc > W) continue;          // behind the last row / column a tap of this frame reaches: never read
            f32x4 v[NV];
            unit16<T>::ld(x + ((int64_t)blur_refl(r, H) * W + blur_refl(cc, W)) * C + c, v);
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                if (AFF) v[q] = relu4(fma4(v[q], s[q], t[q]));
                *reinterpret_cast<f32x4*>(&tile[p][u * V + 4 * q]) = v[q];
            }
        }
        __syncthreads();
#pragma unroll
        for (int o = p0; o < BL_TH * BL_TW; o += PP) {
            const int oi = o / BL_TW, oj = o % BL_TW;
            if (i0 + oi >= Ho || j0 + oj >= Wo) continue;
            f32x4 out[NV];
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const float* b = &tile[2 * oi * BL_HW + 2 * oj][u * V + 4 * q];
                f32x4 h[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const float* rr = b + d * BL_HW * BL_CH;
                    h[d] = tap121(lds4(rr), lds4(rr + BL_CH), lds4(rr + 2 * BL_CH));
                }
                out[q] = tap121(h[0], h[1], h[2]) * 0.0625f;
            }
            unit16<T>::st(y + ((int64_t)(i0 + oi) * Wo + j0 + oj) * C + c, out);
        }
        __syncthreads();
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
// One axis of the transposed stencil as a gather: full-resolution index g (of n; no = ceil(n / 2) outputs) takes wa gy[i] + wb gy[i + 1]
// with i = g >> 1.  Even g is the centre tap of output i alone.  Odd g is the last tap of i and the first of i + 1 (where there is
// one); the row reflected from -1 lands on g = 1 as a second last tap of output 0, the row reflected from n (n odd) on g = n - 2
// as a second first tap of output no - 1.
struct BlurTap { float wa, wb; };
__device__ __forceinline__ BlurTap blur_tap(int g, int n, int no) {
    BlurTap t;
    if (!(g & 1)) { t.wa = 2.f; t.wb = 0.f; return t; }
    t.wa = g == 1 ? 2.f : 1.f;
    t.wb = (g >> 1) + 1 < no ? (((n & 1) && g == n - 2) ? 2.f : 1.f) : 0.f;
    return t;
}

// blurT(gy) at one full-resolution position from the staged halo: `g` points at gy[i][j] of the unit's four channels
__device__ __forceinline__ f32x4 blur_gather(const float* g, BlurTap tr, BlurTap tc) {
    const f32x4 wa = splat4(tc.wa), wb = splat4(tc.wb);
    const f32x4 t0 = fma4(wb, lds4(g + BL_CH), wa * lds4(g));
    const f32x4 t1 = fma4(wb, lds4(g + (BL_GW + 1) * BL_CH), wa * lds4(g + BL_GW * BL_CH));
    return fma4(splat4(tr.wb), t1, splat4(tr.wa) * t0) * 0.0625f;
}
__device__ __forceinline__ f32x4 keep_pos4(f32x4 g, f32x4 a) {
    return f32x4{a.x > 0.f ? g.x : 0.f, a.y > 0.f ? g.y : 0.f, a.z > 0.f ? g.z : 0.f, a.w > 0.f ? g.w : 0.f};
}

enum { BLUR_REDUCE = 0, BLUR_APPLY = 1, BLUR_PLAIN = 2 };

// a, b, cf: REDUCE scale, shift, mean; APPLY scale, shift and k = [k1 | k2 | k3][C]; PLAIN unused.  `xin`: the conv output x
// (REDUCE, APPLY) or the optional addend (PLAIN).  H, W: the FULL resolution
template <int MODE, typename T>
__global__ __launch_bounds__(256) void blur_bwd_kernel(const T* gy, const T* xin, const float* a, const float* b, const float* cf,
                                                       T* gx, double* part, int H, int W, int Ho, int Wo, int C, int tiles_w) {
    constexpr int V = unit16<T>::V, NV = unit16<T>::NV, CU = BL_CH / V, PP = 256 / CU;
    constexpr int FW = 2 * BL_TW, NPOS = 4 * BL_TH * BL_TW, NPASS = NPOS / PP;
    typedef typename unit16<T>::raw_t raw_t;
    __shared__ __attribute__((aligned(16))) float gt[BL_GH * BL_GW][BL_CH];
    __shared__ double red[MODE == BLUR_REDUCE ? 4 : 1][MODE == BLUR_REDUCE ? 256 : 1];
    const int tid = threadIdx.x, u = tid % CU, p0 = tid / CU;
    const int i0 = (int)(blockIdx.x / tiles_w) * BL_TH, j0 = (int)(blockIdx.x % tiles_w) * BL_TW;
    const int64_t full = (int64_t)blockIdx.y * H * W * C;
    gy += (int64_t)blockIdx.y * Ho * Wo * C;
    if (MODE != BLUR_PLAIN || xin) xin += full;
    if (MODE != BLUR_REDUCE) gx += full;
    if (MODE == BLUR_REDUCE) part += ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * C;
    for (int ch = blockIdx.z * BL_CH; ch < C; ch += gridDim.z * BL_CH) {
        const int c = ch + u * V;
        // the thread's full-resolution units first: their loads are in flight while the halo of gy is staged
        raw_t xr[NPASS];
        if (MODE != BLUR_PLAIN || xin) {
#pragma unroll
            for (int k = 0; k < NPASS; ++k) {
                const int p = p0 + k * PP, r = 2 * i0 + p / FW, cc = 2 * j0 + p % FW;
                if (r < H && cc < W) xr[k] = unit16<T>::ldr(xin + ((int64_t)r * W + cc) * C + c);
            }
        }
        for (int p = p0; p < BL_GH * BL_GW; p += PP) {
            const int gi = i0 + p / BL_GW, gj = j0 + p % BL_GW;
            f32x4 v[NV];
#pragma unroll
            for (int q = 0; q < NV; ++q) v[q] = splat4(0.f);
            if (gi < Ho && gj < Wo) unit16<T>::ld(gy + ((int64_t)gi * Wo + gj) * C + c, v);
#pragma unroll
            for (int q = 0; q < NV; ++q) *reinterpret_cast<f32x4*>(&gt[p][u * V + 4 * q]) = v[q];
        }
        f32x4 ca[NV], cb[NV], cc3[NV], ck2[NV], ck3[NV], acc[2][NV];
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            if (MODE != BLUR_PLAIN) { ca[q] = ld4(a + c + 4 * q); cb[q] = ld4(b + c + 4 * q); cc3[q] = ld4(cf + c + 4 * q); }
            if (MODE == BLUR_APPLY) { ck2[q] = ld4(cf + C + c + 4 * q); ck3[q] = ld4(cf + 2 * C + c + 4 * q); }
            acc[0][q] = acc[1][q] = splat4(0.f);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NPASS; ++k) {
            const int p = p0 + k * PP, lr = p / FW, lc = p % FW, r = 2 * i0 + lr, cc = 2 * j0 + lc;
            if (r >= H || cc >= W) continue;
            const BlurTap tr = blur_tap(r, H, Ho), tc = blur_tap(cc, W, Wo);
            const float* g = &gt[(lr >> 1) * BL_GW + (lc >> 1)][u * V];
            f32x4 xv[NV], o[NV];
            if (MODE != BLUR_PLAIN || xin) unit16<T>::cvt(xr[k], xv);
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                f32x4 gz = blur_gather(g + 4 * q, tr, tc);
                if (MODE == BLUR_PLAIN) {
                    o[q] = xin ? xv[q] + gz : gz;
                } else {
                    gz = keep_pos4(gz, fma4(xv[q], ca[q], cb[q]));
                    if (MODE == BLUR_REDUCE) {
                        acc[0][q] += gz;
                        acc[1][q] = fma4(gz, xv[q] - cc3[q], acc[1][q]);
                    } else {
                        o[q] = fma4(cc3[q], gz, fma4(ck2[q], xv[q], ck3[q]));
                    }
                }
            }
            if (MODE != BLUR_REDUCE) unit16<T>::st(gx + ((int64_t)r * W + cc) * C + c, o);
        }
        if (MODE == BLUR_REDUCE) {
            // fp64 across the PP threads that share the channel unit (tid = u + p0 CU), a halving tree in a fixed order
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int q = 0; q < NV; ++q) {
                    red[0][tid] = (double)acc[n][q].x; red[1][tid] = (double)acc[n][q].y;
                    red[2][tid] = (double)acc[n][q].z; red[3][tid] = (double)acc[n][q].w;
                    for (int s = PP / 2; s > 0; s >>= 1) {
                        __syncthreads();
                        if (p0 < s) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) red[e][tid] += red[e][tid + s * CU];
                        }
                    }
                    if (p0 == 0) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) part[(size_t)n * C + c + 4 * q + e] = red[e][tid];
                    }
                    __syncthreads();
                }
        }
        __syncthreads();
    }
}

// sums[e] = the records' entries e = (n, c) added in record order: 16 lanes per entry walk the records 16 apart, then a fixed tree
__global__ __launch_bounds__(256) void blur_fold_kernel(const double* part, double* sums, int nrec, int E) {
    __shared__ double red[256];
    const int tid = threadIdx.x, e = blockIdx.x * 16 + (tid & 15), l = tid >> 4;
    double a = 0.0;
    for (int k = l; k < nrec; k += 16) a += part[(size_t)k * E + e];
    red[tid] = a;
    for (int s = 8; s > 0; s >>= 1) {
        __syncthreads();
        if (l < s) red[tid] += red[tid + 16 * s];
    }
    if (l == 0) sums[e] = red[tid];
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------------
struct BlurPlan { int Ho, Wo, tiles_w, tiles, gz; };

// H, W: the full resolution.  Every channel count that is a multiple of 64 up to 2048; both tensors in one storage type
static inline int blur_plan(int32_t B, int32_t H, int32_t W, int32_t C, int32_t bytes_a, int32_t bytes_b, BlurPlan* p) {
    if (B <= 0 || H < 2 || W < 2 || C < BL_CH || C > BL_MAX_C || C % BL_CH) return LOANS_EINVAL;
    if (bytes_a != bytes_b || (bytes_a != 4 && bytes_a != 2)) return LOANS_EINVAL;
    if (B > 65535 || H > (1 << 15) || W > (1 << 15)) return LOANS_ERANGE;
    p->Ho = (H + 1) / 2; p->Wo = (W + 1) / 2;
    p->tiles_w = (p->Wo + BL_TW - 1) / BL_TW;
    p->tiles = p->tiles_w * ((p->Ho + BL_TH - 1) / BL_TH);
    p->gz = C / BL_CH < BL_MAX_Z ? C / BL_CH : BL_MAX_Z;
    return LOANS_OK;
}
static inline bool mis16(const void* p) { return ((uintptr_t)p & 15) != 0; }

template <typename T>
static void blur_fwd_launch(const void* x, const float* scale, const float* shift, void* y, int B, int H, int W, int C,
                            const BlurPlan& p, hipStream_t st) {
    const dim3 grid(p.tiles, B, p.gz);
    if (scale)
        hipLaunchKernelGGL((blur_fwd_kernel<true, T>), grid, dim3(256), 0, st, static_cast<const T*>(x), scale, shift,
                           static_cast<T*>(y), H, W, p.Ho, p.Wo, C, p.tiles_w);
    else
        hipLaunchKernelGGL((blur_fwd_kernel<false, T>), grid, dim3(256), 0, st, static_cast<const T*>(x), scale, shift,
                           static_cast<T*>(y), H, W, p.Ho, p.Wo, C, p.tiles_w);
}

template <int MODE, typename T>
static void blur_bwd_launch(const void* gy, const void* xin, const float* a, const float* b, const float* cf, void* gx, double* part,
                            int B, int H, int W, int C, const BlurPlan& p, hipStream_t st) {
    hipLaunchKernelGGL((blur_bwd_kernel<MODE, T>), dim3(p.tiles, B, p.gz), dim3(256), 0, st, static_cast<const T*>(gy),
                       static_cast<const T*>(xin), a, b, cf, static_cast<T*>(gx), part, H, W, p.Ho, p.Wo, C, p.tiles_w);
}

}  // namespace

extern "C" int loans_blur_fwd(const void* x, const float* scale, const float* shift, void* y, int32_t B, int32_t H, int32_t W,
                              int32_t C, int32_t x_bytes, int32_t y_bytes, void* stream) {
    BlurPlan p;
    if (int rc = blur_plan(B, H, W, C, x_bytes, y_bytes, &p)) return rc;
    if (!x || !y || (scale == nullptr) != (shift == nullptr) || mis16(x) || mis16(y) || mis16(scale) || mis16(shift)) return LOANS_EINVAL;
    if (x_bytes == 4) blur_fwd_launch<float>(x, scale, shift, y, B, H, W, C, p, as_stream(stream));
    else blur_fwd_launch<__bf16>(x, scale, shift, y, B, H, W, C, p, as_stream(stream));
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_blur_bwd_records(int32_t B, int32_t H, int32_t W) {
    BlurPlan p;
    if (int rc = blur_plan(B, H, W, BL_CH, 4, 4, &p)) return rc;
    return (int64_t)B * p.tiles > (1 << 30) ? LOANS_ERANGE : B * p.tiles;
}

extern "C" int loans_blur_bwd_reduce(const void* gy, const void* x, const float* scale, const float* shift, const float* mean,
                                     double* partial, double* sums, int32_t B, int32_t H, int32_t W, int32_t C, int32_t gy_bytes,
                                     int32_t x_bytes, void* stream) {
    BlurPlan p;
    if (int rc = blur_plan(B, H, W, C, gy_bytes, x_bytes, &p)) return rc;
    if (!gy || !x || !scale || !shift || !mean || !partial || !sums) return LOANS_EINVAL;
    if (mis16(gy) || mis16(x) || mis16(scale) || mis16(shift) || mis16(mean) || ((uintptr_t)partial & 7) || ((uintptr_t)sums & 7))
        return LOANS_EINVAL;
    if ((int64_t)B * p.tiles > (1 << 30)) return LOANS_ERANGE;
    hipStream_t st = as_stream(stream);
    if (x_bytes == 4) blur_bwd_launch<BLUR_REDUCE, float>(gy, x, scale, shift, mean, nullptr, partial, B, H, W, C, p, st);
    else blur_bwd_launch<BLUR_REDUCE, __bf16>(gy, x, scale, shift, mean, nullptr, partial, B, H, W, C, p, st);
    LOANS_LAUNCH_CHECK();
    hipLaunchKernelGGL(blur_fold_kernel, dim3(2 * C / 16), dim3(256), 0, st, partial, sums, B * p.tiles, 2 * C);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_blur_bwd_apply(const void* gy, const void* x, const float* scale, const float* shift, const float* k, void* gx,
                                    int32_t B, int32_t H, int32_t W, int32_t C, int32_t gy_bytes, int32_t x_bytes, void* stream) {
    BlurPlan p;
    if (int rc = blur_plan(B, H, W, C, gy_bytes, x_bytes, &p)) return rc;
    if (!gy || !x || !scale || !shift || !k || !gx) return LOANS_EINVAL;
    if (mis16(gy) || mis16(x) || mis16(scale) || mis16(shift) || mis16(k) || mis16(gx)) return LOANS_EINVAL;
    hipStream_t st = as_stream(stream);
    if (x_bytes == 4) blur_bwd_launch<BLUR_APPLY, float>(gy, x, scale, shift, k, gx, nullptr, B, H, W, C, p, st);
    else blur_bwd_launch<BLUR_APPLY, __bf16>(gy, x, scale, shift, k, gx, nullptr, B, H, W, C, p, st);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_blur_bwd_plain(const void* gy, const void* addend, void* gx, int32_t B, int32_t H, int32_t W, int32_t C,
                                    int32_t gy_bytes, int32_t gx_bytes, void* stream) {
    BlurPlan p;
    if (int rc = blur_plan(B, H, W, C, gy_bytes, gx_bytes, &p)) return rc;
    if (!gy || !gx || mis16(gy) || mis16(addend) || mis16(gx)) return LOANS_EINVAL;
    hipStream_t st = as_stream(stream);
    if (gx_bytes == 4) blur_bwd_launch<BLUR_PLAIN, float>(gy, addend, nullptr, nullptr, nullptr, gx, nullptr, B, H, W, C, p, st);
    else blur_bwd_launch<BLUR_PLAIN, __bf16>(gy, addend, nullptr, nullptr, nullptr, gx, nullptr, B, H, W, C, p, st);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}
