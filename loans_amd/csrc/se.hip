// Squeeze-and-excitation at a residual unit's junction (Hu et al. 2018; functions/blocks.py, links.SqueezeExcite):
//     q[b,c] = mean_p bn(c)[b,p,c]      h = relu(W1 q + b1)      s = sigmoid(W2 h + b2)      y = relu(s[b,c] bn(c) + second)
// The tensors are [B][P][C] (NHWC, P = Ho * Wo).  The squeeze is linear in c, so it is ONE read of the conv output (S = sum_p c,
// q = scale S / P + shift), and the whole backward of the junction is one reduction pass that leaves per-(sample, channel) tables
// (G0 = sum_p g, G1 = sum_p g c, G2 = sum_p g c2), a per-sample kernel on those tables, and one apply pass: the pass count of
// the ungated junction (bn_pool.hip's rows kernels).
//
// How the streaming kernels split the work: a block owns a slab of ONE sample's units (16 bytes: 4 fp32 / 8 bf16 channels), grid
// (slabs per sample, B, channel chunks).  With U = C / V units per row,
//   U <= 256 dividing 256 ... the slab is contiguous, a multiple of 256 units: thread tid keeps channel unit tid % U, the 256 / U
//                             threads that share a channel unit meet in LDS in a halving tree
//   U a multiple of 256 ..... blockIdx.z picks 256 of a row's units and the block walks rows: every thread owns its channels
// so the gate row s[b][.] of a thread's channels sits in registers for the whole slab, and no index is ever divided.  A sample of
// 7 x 7 positions is one block, one of 56 x 56 many: the blocks of a sample leave partial records [B][slabs][..] that a second
// small launch folds in slab order.  No floating-point atomics anywhere in this file: two runs give the same bits.
#include "common.h"
#include "unit16.h"

namespace {

template <typename T> static inline int se_units(int C) {
    constexpr int V = unit16<T>::V;
    if (C <= 0 || C % V) return 0;
    const int U = C / V;
    return ((U <= 256 && 256 % U == 0) || U % 256 == 0) ? U : 0;
}

// G slabs per sample, gz channel chunks, `per` units of a sample per block (a multiple of 256 or of U), thread stride `step`
struct SePlan { int G, gz, step; int64_t per; };
static inline SePlan se_plan(int B, int64_t P, int U) {
    SePlan p;
    if (U <= 256) {
        const int64_t nps = P * U;
        p.gz = 1; p.step = 256;
        const int64_t cap = 8192 / B > 0 ? 8192 / B : 1;
        int64_t g = (nps + 256 * SLAB_UNR - 1) / (256 * SLAB_UNR);
        if (g > cap) g = cap;
        p.per = ((nps + g - 1) / g + 255) & ~(int64_t)255;
        p.G = (int)((nps + p.per - 1) / p.per);
    } else {
        p.gz = U / 256; p.step = U;
        const int64_t cap = 8192 / ((int64_t)B * p.gz) > 0 ? 8192 / ((int64_t)B * p.gz) : 1;
        int64_t g = (P + SLAB_UNR - 1) / SLAB_UNR;
        if (g > cap) g = cap;
        const int64_t rpb = (P + g - 1) / g;
        p.per = rpb * U;
        p.G = (int)((P + rpb - 1) / rpb);
    }
    return p;
}

template <typename T> static inline int se_check(int32_t B, int64_t P, int32_t C, int* U) {
    if (B <= 0 || P <= 0 || !(*U = se_units<T>(C))) return LOANS_EINVAL;
    if (P * *U >= ((int64_t)1 << 30) || B > 65535) return LOANS_ERANGE;
    return LOANS_OK;
}
static inline bool mis16(const void* p) { return ((uintptr_t)p & 15) != 0; }

// the units of the block's slab a thread visits: i, i + step, ... < end inside sample blockIdx.y (unit index in the sample)
struct SeWalk { int64_t i, end; int cu; };
__device__ __forceinline__ SeWalk se_walk(int64_t nps, int64_t per, int U) {
    const int64_t lo = (int64_t)blockIdx.x * per;
    SeWalk w;
    w.i = lo + blockIdx.z * 256 + threadIdx.x;
    w.end = lo + per < nps ? lo + per : nps;
    w.cu = (blockIdx.z * 256 + threadIdx.x) % U;
    return w;
}

// block tree over the RL = 256 / U threads that share a channel unit (tid = cu + k U); the sum ends at tid < U
template <typename A> __device__ __forceinline__ void se_tree(A* red, int U) {
    const int tid = threadIdx.x;
    for (int s = 128 / U; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s * U) red[tid] += red[tid + s * U];
    }
    __syncthreads();
}

// ---- 1. squeeze: part[b][slab][C] = the slab's sums of x over positions ------------------------------------------------------
template <bool NT, typename T>
__global__ __launch_bounds__(256) void se_squeeze_kernel(const T* x, float* part, int64_t nps, int U, int step, int64_t per) {
    constexpr int V = unit16<T>::V, NV = unit16<T>::NV;
    typedef typename unit16<T>::raw_t raw_t;
    __shared__ f32x4 red[256];
    const SeWalk w = se_walk(nps, per, U);
    x += (int64_t)blockIdx.y * nps * V;
    f32x4 acc[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    int64_t i = w.i;
    for (; i + (int64_t)(SLAB_UNR - 1) * step < w.end; i += (int64_t)SLAB_UNR * step) {
        raw_t a[SLAB_UNR];
#pragma unroll
        for (int u = 0; u < SLAB_UNR; ++u) a[u] = unit16<T>::template ldr<NT>(x + (i + (int64_t)u * step) * V);
#pragma unroll
        for (int u = 0; u < SLAB_UNR; ++u) {
            f32x4 v[NV];
            unit16<T>::cvt(a[u], v);
#pragma unroll
            for (int q = 0; q < NV; ++q) acc[q] += v[q];
        }
    }
    for (; i < w.end; i += step) {
        f32x4 v[NV];
        unit16<T>::cvt(unit16<T>::template ldr<NT>(x + i * V), v);
#pragma unroll
        for (int q = 0; q < NV; ++q) acc[q] += v[q];
    }
    const int C = U * V, owners = U < 256 ? U : 256;
    part += ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * C + w.cu * V;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        if (U < 256) {
            red[threadIdx.x] = acc[q];
            se_tree(red, U);
            acc[q] = red[threadIdx.x];
            __syncthreads();
        }
        if ((int)threadIdx.x < owners) *reinterpret_cast<f32x4*>(part + 4 * q) = acc[q];
    }
}

// out_n[b][c] = sum over slabs, in slab order, of part[b][slab][n][c], n < NS (fp32 or fp64 records, fp32 tables)
template <typename TI>
__global__ void se_fold_kernel(const TI* part, float* o0, float* o1, float* o2, int B, int G, int NS, int C) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)B * NS * C) return;
    const int c = (int)(idx % C), n = (int)(idx / C % NS), b = (int)(idx / ((int64_t)C * NS));
    const TI* p = part + ((size_t)b * G * NS + n) * C + c;
    TI a = 0;
    for (int k = 0; k < G; ++k) a += p[(size_t)k * NS * C];
    float* o = n == 0 ? o0 : (n == 1 ? o1 : o2);
    o[(size_t)b * C + c] = (float)a;
}

// ---- 2. excitation forward: one block per sample ---------------------------------------------------------------------------------
// a row of n4 float4s against a vector in LDS, GW lanes per row (a power of two <= 64), folded with shuffles inside the group
__device__ __forceinline__ float group_dot(const float* row, const float* vec, int n4, int GW, int l) {
    f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = l; k < n4; k += GW) a += ld4(row + 4 * k) * *reinterpret_cast<const f32x4*>(vec + 4 * k);
    float s = (a.x + a.y) + (a.z + a.w);
    for (int o = GW >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}
__device__ __forceinline__ int group_width(int n4) {
    int g = 1;
    while (g < n4 && g < 64) g <<= 1;
    return g;
}
// 1 / (1 + exp(-a)), finite for every finite a
__device__ __forceinline__ float sigmoidf(float a) {
    const float e = __expf(-fabsf(a));
    return a >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

constexpr int SE_MAX_C = 2048, SE_MAX_H = 512;

__global__ __launch_bounds__(256) void se_excite_fwd_kernel(const float* S, const float* scale, const float* shift, const float* W1,
                                                            const float* b1, const float* W2, const float* b2, float* s, float* h,
                                                            float* q, int C, int Ch, float inv_p) {
    __shared__ __attribute__((aligned(16))) float ql[SE_MAX_C];
    __shared__ __attribute__((aligned(16))) float hl[SE_MAX_H];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int c = tid; c < C; c += 256) {
        const float v = scale[c] * (S[(size_t)b * C + c] * inv_p) + shift[c];
        ql[c] = v;
        q[(size_t)b * C + c] = v;
    }
    __syncthreads();
    {   // h = relu(W1 q + b1): W1 [Ch][C]
        const int GW = group_width(C / 4), RPW = 64 / GW, l = lane % GW;
        for (int r0 = wave * RPW; r0 < Ch; r0 += 4 * RPW) {
            const int r = r0 + lane / GW, rr = r < Ch ? r : Ch - 1;
            const float v = fmaxf(group_dot(W1 + (size_t)rr * C, ql, C / 4, GW, l) + b1[rr], 0.f);
            if (r < Ch && l == 0) { hl[r] = v; h[(size_t)b * Ch + r] = v; }
        }
    }
    __syncthreads();
    {   // s = sigmoid(W2 h + b2): W2 [C][Ch]
        const int GW = group_width(Ch / 4), RPW = 64 / GW, l = lane % GW;
        for (int r0 = wave * RPW; r0 < C; r0 += 4 * RPW) {
            const int r = r0 + lane / GW, rr = r < C ? r : C - 1;
            const float v = sigmoidf(group_dot(W2 + (size_t)rr * Ch, hl, Ch / 4, GW, l) + b2[rr]);
            if (r < C && l == 0) s[(size_t)b * C + r] = v;
        }
    }
}

// ---- 3. gated junction forward: y = relu(s[b][c] (x scale + shift) + second), sign bits always -------------------------------
template <int MODE, bool NT, typename T>
__global__ __launch_bounds__(256) void bn_apply_gate_kernel(const T* x, const float* scale, const float* shift, const T* x2,
                                                            const float* scale2, const float* shift2, const float* gate, T* y,
                                                            uint8_t* signbits, int64_t nps, int U, int step, int64_t per) {
    constexpr int V = unit16<T>::V, NV = unit16<T>::NV;
    typedef typename unit16<T>::raw_t raw_t;
    const SeWalk w = se_walk(nps, per, U);
    const int64_t base = (int64_t)blockIdx.y * nps;
    x += base * V; x2 += base * V; y += base * V; signbits += base * NV;
    gate += (size_t)blockIdx.y * U * V + w.cu * V;
    f32x4 s[NV], t[NV], s2[NV], t2[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const f32x4 g = ld4(gate + 4 * q);            // the gate folded into the coefficients: s (x scale + shift)
        s[q] = g * ld4(scale + w.cu * V + 4 * q); t[q] = g * ld4(shift + w.cu * V + 4 * q);
        if (MODE == 2) { s2[q] = ld4(scale2 + w.cu * V + 4 * q); t2[q] = ld4(shift2 + w.cu * V + 4 * q); }
    }
    auto one = [&](int64_t i, raw_t xr, raw_t rr) {
        f32x4 v[NV], xv[NV], sv[NV];
        unit16<T>::cvt(xr, xv);
        unit16<T>::cvt(rr, sv);
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            if (MODE == 2) sv[q] = sv[q] * s2[q] + t2[q];
            v[q] = relu4((xv[q] * s[q] + t[q]) + sv[q]);
        }
        unit16<T>::template st<NT>(y + i * V, v);
        st_bits<NV>(signbits + i * NV, v);
    };
    int64_t i = w.i;
    for (; i + (int64_t)(SLAB_UNR - 1) * step < w.end; i += (int64_t)SLAB_UNR * step) {
        raw_t a[SLAB_UNR], r[SLAB_UNR];
#pragma unroll
        for (int u = 0; u < SLAB_UNR; ++u) {
            const int64_t j = i + (int64_t)u * step;
            a[u] = unit16<T>::template ldr<NT>(x + j * V);
            r[u] = unit16<T>::template ldr<NT>(x2 + j * V);
        }
#pragma unroll
        for (int u = 0; u < SLAB_UNR; ++u) one(i + (int64_t)u * step, a[u], r[u]);
    }
    for (; i < w.end; i += step) one(i, unit16<T>::template ldr<NT>(x + i * V), unit16<T>::template ldr<NT>(x2 + i * V));
}

// ---- 4. backward reduction: part[b][slab][NS][C] (fp64) = the slab's [sum g | sum g x | sum g x2], g = gy * bit --------------
template <bool DUAL, typename T>
__global__ __launch_bounds__(256) void se_bwd_reduce_kernel(const T* gy, const uint8_t* bits, const T* x, const T* x2, double* part,
                                                            int64_t nps, int U, int step, int64_t per) {
    constexpr int V = unit16<T>::V, NV = unit16<T>::NV, NS = DUAL ? 3 : 2;
    typedef typename unit16<T>::raw_t raw_t;
    __shared__ double red[4][256];
    const SeWalk w = se_walk(nps, per, U);
    const int64_t base = (int64_t)blockIdx.y * nps;
    gy += base * V; x += base * V; bits += base * NV;
    if (DUAL) x2 += base * V;
    f32x4 acc[NS][NV];
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
        for (int q = 0; q < NV; ++q) acc[n][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto fold = [&](raw_t gr, raw_t xr, raw_t wr, const uint8_t* mb) {
        f32x4 g[NV], xv[NV], xw[NV];
        unit16<T>::cvt(gr, g);
        unit16<T>::cvt(xr, xv);
        if (DUAL) unit16<T>::cvt(wr, xw);
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            g[q] = maskbits4(g[q], mb[q]);
            acc[0][q] += g[q];
            acc[1][q] += g[q] * xv[q];
            if (DUAL) acc[2][q] += g[q] * xw[q];
        }
    };
    constexpr int UF = DUAL ? 2 : 4;
    int64_t i = w.i;
    for (; i + (int64_t)(UF - 1) * step < w.end; i += (int64_t)UF * step) {
        raw_t g[UF], xv[UF], xw[UF];
        uint8_t mb[UF][NV];
#pragma unroll
        for (int u = 0; u < UF; ++u) {
            const int64_t j = i + (int64_t)u * step;
            g[u] = unit16<T>::ldr(gy + j * V);
            xv[u] = unit16<T>::ldr(x + j * V);
            xw[u] = DUAL ? unit16<T>::ldr(x2 + j * V) : g[u];
            ld_bits<NV>(bits + j * NV, mb[u]);
        }
#pragma unroll
        for (int u = 0; u < UF; ++u) fold(g[u], xv[u], xw[u], mb[u]);
    }
    for (; i < w.end; i += step) {
        const raw_t g = unit16<T>::ldr(gy + i * V), xv = unit16<T>::ldr(x + i * V), xw = DUAL ? unit16<T>::ldr(x2 + i * V) : g;
        uint8_t mb[NV];
        ld_bits<NV>(bits + i * NV, mb);
        fold(g, xv, xw, mb);
    }
    const int C = U * V, tid = threadIdx.x, owners = U < 256 ? U : 256;
    part += ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NS * C + w.cu * V;
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            double d[4] = {(double)acc[n][q].x, (double)acc[n][q].y, (double)acc[n][q].z, (double)acc[n][q].w};
            if (U < 256) {          // fp64 across the block's tree, the four channels of the vector side by side
#pragma unroll
                for (int e = 0; e < 4; ++e) red[e][tid] = d[e];
                for (int s = 128 / U; s > 0; s >>= 1) {
                    __syncthreads();
                    if (tid < s * U) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) red[e][tid] += red[e][tid + s * U];
                    }
                }
                __syncthreads();
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = red[e][tid];
                __syncthreads();
            }
            if (tid < owners) {
#pragma unroll
                for (int e = 0; e < 4; ++e) part[(size_t)n * C + 4 * q + e] = d[e];
            }
        }
}

// ---- 5. excitation backward -------------------------------------------------------------------------------------------------------
// per sample: ds = scale G1 + shift G0, da2 = ds s (1 - s), dh = (W2^T da2) (h > 0), dq = W1^T dh, t = dq / P, and the sample's
// terms of the last BN's two sums, u0 = s G0 + dq, u1 = s (G1 - mean G0) + t (S - P mean)  (fp64)
__global__ __launch_bounds__(256) void se_excite_bwd_kernel(const float* G0, const float* G1, const float* S, const float* scale,
                                                            const float* shift, const float* mean, const float* s, const float* h,
                                                            const float* W1, const float* W2, float* t, float* da2, float* dh,
                                                            double* u, int C, int Ch, float inv_p, float P) {
    __shared__ float al[SE_MAX_C];
    __shared__ float dl[SE_MAX_H];
    __shared__ float pl[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t bc = (size_t)b * C;
    for (int c = tid; c < C; c += 256) {
        const float sv = s[bc + c];
        const float a = (scale[c] * G1[bc + c] + shift[c] * G0[bc + c]) * sv * (1.f - sv);
        al[c] = a;
        da2[bc + c] = a;
    }
    __syncthreads();
    int JW = 1;                                     // threads side by side over the hidden units, NP parts of the channels each
    while (JW < Ch && JW < 256) JW <<= 1;
    const int NP = 256 / JW, jj = tid % JW, pt = tid / JW;
    for (int j0 = 0; j0 < Ch; j0 += JW) {
        const int j = j0 + jj;
        float a = 0.f;
        if (j < Ch)
            for (int c = pt; c < C; c += NP) a += W2[(size_t)c * Ch + j] * al[c];
        pl[tid] = a;
        __syncthreads();
        if (pt == 0 && j < Ch) {
            for (int k = 1; k < NP; ++k) a += pl[k * JW + jj];
            a = h[(size_t)b * Ch + j] > 0.f ? a : 0.f;
            dl[j] = a;
            dh[(size_t)b * Ch + j] = a;
        }
        __syncthreads();
    }
    for (int c = tid; c < C; c += 256) {
        float dq = 0.f;
        for (int j = 0; j < Ch; ++j) dq += W1[(size_t)j * C + c] * dl[j];
        const float tv = dq * inv_p;
        t[bc + c] = tv;
        const double sv = s[bc + c], g0 = G0[bc + c], g1 = G1[bc + c], mu = mean[c];
        u[2 * bc + c] = sv * g0 + (double)dq;
        u[2 * bc + C + c] = sv * (g1 - mu * g0) + (double)tv * ((double)S[bc + c] - (double)P * mu);
    }
}

// over the batch, in sample order: gW2 += da2^T h, gW1 += dh^T q, gb2 += sum da2, gb1 += sum dh, and replica 0 of the BN sums
// [sum gz | sum gz xhat] (DUAL: + [sum g | sum g xhat2]) in loans_bn_bwd_coeffs_rep_f32's layout
__global__ __launch_bounds__(256) void se_excite_bwd_fold_kernel(const float* da2, const float* dh, const float* h, const float* q,
                                                                 const double* u, const float* rstd, const float* G0, const float* G2,
                                                                 const float* mean2, const float* rstd2, float* gW1, float* gb1,
                                                                 float* gW2, float* gb2, double* sums, int B, int C, int Ch) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nw = (int64_t)C * Ch;
    double a = 0.0;
    if (idx < nw) {
        const int c = (int)(idx / Ch), j = (int)(idx % Ch);
        for (int b = 0; b < B; ++b) a += (double)da2[(size_t)b * C + c] * (double)h[(size_t)b * Ch + j];
        gW2[idx] += (float)a;
        return;
    }
    idx -= nw;
    if (idx < nw) {
        const int j = (int)(idx / C), c = (int)(idx % C);
        for (int b = 0; b < B; ++b) a += (double)dh[(size_t)b * Ch + j] * (double)q[(size_t)b * C + c];
        gW1[idx] += (float)a;
        return;
    }
    idx -= nw;
    if (idx < C) {
        for (int b = 0; b < B; ++b) a += (double)da2[(size_t)b * C + idx];
        gb2[idx] += (float)a;
        return;
    }
    idx -= C;
    if (idx < Ch) {
        for (int b = 0; b < B; ++b) a += (double)dh[(size_t)b * Ch + idx];
        gb1[idx] += (float)a;
        return;
    }
    idx -= Ch;
    if (idx < 2 * C) {
        const int n = (int)(idx / C), c = (int)(idx % C);
        for (int b = 0; b < B; ++b) a += u[((size_t)b * 2 + n) * C + c];
        sums[idx] = n ? (double)rstd[c] * a : a;
        return;
    }
    idx -= 2 * C;
    if (G2 && idx < 2 * C) {
        const int n = (int)(idx / C), c = (int)(idx % C);
        const double mu = mean2[c];
        for (int b = 0; b < B; ++b) {
            const double g0 = G0[(size_t)b * C + c];
            a += n ? (double)G2[(size_t)b * C + c] - mu * g0 : g0;
        }
        sums[2 * C + idx] = n ? (double)rstd2[c] * a : a;
    }
}

// ---- 6. gated junction backward: gx = k1 (s[b][c] g + t[b][c]) + k2 x + k3, DUAL: gx2 = k1b g + k2b x2 + k3b -----------------
template <bool DUAL, bool NT, typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_gate_kernel(const T* gy, const uint8_t* bits, const float* gate, const float* tt,
                                                                const T* x, const float* k1, const float* k2, const float* k3, T* gx,
                                                                const T* x2, const float* k1b, const float* k2b, const float* k3b,
                                                                T* gx2, int64_t nps, int U, int step, int64_t per) {
    constexpr int V = unit16<T>::V, NV = unit16<T>::NV;
    typedef typename unit16<T>::raw_t raw_t;
    const SeWalk w = se_walk(nps, per, U);
    const int64_t base = (int64_t)blockIdx.y * nps;
    gy += base * V; x += base * V; gx += base * V; bits += base * NV;
    if (DUAL) { x2 += base * V; gx2 += base * V; }
    const size_t bc = (size_t)blockIdx.y * U * V + w.cu * V;
    f32x4 a1[NV], a2[NV], a3[NV], b1[NV], b2[NV], b3[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const int c = w.cu * V + 4 * q;
        const f32x4 k = ld4(k1 + c);                  // gx = (k1 s) g + k2 x + (k1 t + k3)
        a1[q] = k * ld4(gate + bc + 4 * q); a2[q] = ld4(k2 + c); a3[q] = k * ld4(tt + bc + 4 * q) + ld4(k3 + c);
        if (DUAL) { b1[q] = ld4(k1b + c); b2[q] = ld4(k2b + c); b3[q] = ld4(k3b + c); }
    }
    auto one = [&](int64_t i, raw_t gr, raw_t xr, const uint8_t* mb, raw_t wr) {
        f32x4 o[NV], g[NV], xv[NV], xw[NV];
        unit16<T>::cvt(gr, g);
        unit16<T>::cvt(xr, xv);
        if (DUAL) unit16<T>::cvt(wr, xw);
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            g[q] = maskbits4(g[q], mb[q]);
            o[q] = a1[q] * g[q] + a2[q] * xv[q] + a3[q];
        }
        unit16<T>::template st<NT>(gx + i * V, o);
        if (DUAL) {
#pragma unroll
            for (int q = 0; q < NV; ++q) o[q] = b1[q] * g[q] + b2[q] * xw[q] + b3[q];
            unit16<T>::template st<NT>(gx2 + i * V, o);
        }
    };
    int64_t i = w.i;
    for (; i + (int64_t)(SLAB_UNR - 1) * step < w.end; i += (int64_t)SLAB_UNR * step) {
        raw_t g[SLAB_UNR], xv[SLAB_UNR], xw[SLAB_UNR];
        uint8_t mb[SLAB_UNR][NV];
#pragma unroll
        for (int u = 0; u < SLAB_UNR; ++u) {
            const int64_t j = i + (int64_t)u * step;
            g[u] = unit16<T>::template ldr<NT>(gy + j * V);
            xv[u] = unit16<T>::template ldr<NT>(x + j * V);
            ld_bits<NV>(bits + j * NV, mb[u]);
            xw[u] = DUAL ? unit16<T>::template ldr<NT>(x2 + j * V) : g[u];
        }
#pragma unroll
        for (int u = 0; u < SLAB_UNR; ++u) one(i + (int64_t)u * step, g[u], xv[u], mb[u], xw[u]);
    }
    for (; i < w.end; i += step) {
        const raw_t g = unit16<T>::template ldr<NT>(gy + i * V), xv = unit16<T>::template ldr<NT>(x + i * V);
        const raw_t xw = DUAL ? unit16<T>::template ldr<NT>(x2 + i * V) : g;
        uint8_t mb[NV];
        ld_bits<NV>(bits + i * NV, mb);
        one(i, g, xv, mb, xw);
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------------
template <typename T> static int se_slabs_impl(int32_t B, int64_t P, int32_t C) {
    int U;
    if (int rc = se_check<T>(B, P, C, &U)) return rc;
    return se_plan(B, P, U).G;
}

template <typename T>
static int se_squeeze_impl(const void* x_, float* S, float* part, int32_t B, int64_t P, int32_t C, void* stream) {
    const T* x = static_cast<const T*>(x_);
    if (!x || !S || mis16(x) || mis16(S) || mis16(part)) return LOANS_EINVAL;
    int U;
    if (int rc = se_check<T>(B, P, C, &U)) return rc;
    const SePlan p = se_plan(B, P, U);
    if (p.G > 1 && !part) return LOANS_EINVAL;
    const int64_t nps = P * U;
    float* out = p.G > 1 ? part : S;              // one slab per sample: its record IS the sample's sum
    hipStream_t st = as_stream(stream);
    if (slab_nt((int64_t)B * nps * 16))
        hipLaunchKernelGGL((se_squeeze_kernel<true, T>), dim3(p.G, B, p.gz), dim3(256), 0, st, x, out, nps, U, p.step, p.per);
    else
        hipLaunchKernelGGL((se_squeeze_kernel<false, T>), dim3(p.G, B, p.gz), dim3(256), 0, st, x, out, nps, U, p.step, p.per);
    LOANS_LAUNCH_CHECK();
    if (p.G > 1) {
        hipLaunchKernelGGL((se_fold_kernel<float>), dim3(grid_for((int64_t)B * C, 256, 1 << 30)), dim3(256), 0, st, part, S, S, S, B,
                           p.G, 1, C);
        LOANS_LAUNCH_CHECK();
    }
    return LOANS_OK;
}

static inline int se_hidden_ok(int32_t C, int32_t Ch) {
    return C > 0 && C % 4 == 0 && C <= SE_MAX_C && Ch >= 4 && Ch % 4 == 0 && Ch <= SE_MAX_H;
}

template <typename T>
static int bn_apply_gate_impl(const void* x_, const float* scale, const float* shift, const void* x2_, const float* scale2,
                              const float* shift2, const float* gate, void* y_, uint8_t* signbits, int32_t B, int64_t P, int32_t C,
                              int32_t mode, void* stream) {
    const T *x = static_cast<const T*>(x_), *x2 = static_cast<const T*>(x2_);
    T* y = static_cast<T*>(y_);
    if (!x || !scale || !shift || !x2 || !gate || !y || !signbits) return LOANS_EINVAL;
    if (mode < 1 || mode > 2 || (mode == 2 && (!scale2 || !shift2))) return LOANS_EINVAL;
    if (mis16(x) || mis16(x2) || mis16(y) || mis16(scale) || mis16(shift) || mis16(scale2) || mis16(shift2) || mis16(gate) ||
        ((uintptr_t)signbits & 1))
        return LOANS_EINVAL;
    int U;
    if (int rc = se_check<T>(B, P, C, &U)) return rc;
    const SePlan p = se_plan(B, P, U);
    const int64_t nps = P * U;
    const bool nt = slab_nt((int64_t)B * nps * 16);
    hipStream_t st = as_stream(stream);
#define LAUNCH_AG_(M, N_) hipLaunchKernelGGL((bn_apply_gate_kernel<M, N_, T>), dim3(p.G, B, p.gz), dim3(256), 0, st, x, scale, shift, x2, scale2, shift2, gate, y, signbits, nps, U, p.step, p.per)
#define LAUNCH_AG(M) do { if (nt) LAUNCH_AG_(M, true); else LAUNCH_AG_(M, false); } while (0)
    if (mode == 1) LAUNCH_AG(1); else LAUNCH_AG(2);
#undef LAUNCH_AG
#undef LAUNCH_AG_
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

template <typename T>
static int se_bwd_reduce_impl(const void* gy_, const uint8_t* signbits, const void* x_, const void* x2_, float* G0, float* G1,
                              float* G2, double* part, int32_t B, int64_t P, int32_t C, void* stream) {
    const T *gy = static_cast<const T*>(gy_), *x = static_cast<const T*>(x_), *x2 = static_cast<const T*>(x2_);
    if (!gy || !signbits || !x || !G0 || !G1 || !part || (x2 && !G2)) return LOANS_EINVAL;
    if (mis16(gy) || mis16(x) || mis16(x2) || ((uintptr_t)signbits & 1) || ((uintptr_t)part & 7)) return LOANS_EINVAL;
    int U;
    if (int rc = se_check<T>(B, P, C, &U)) return rc;
    const SePlan p = se_plan(B, P, U);
    const int64_t nps = P * U;
    const int NS = x2 ? 3 : 2;
    hipStream_t st = as_stream(stream);
    if (x2) hipLaunchKernelGGL((se_bwd_reduce_kernel<true, T>), dim3(p.G, B, p.gz), dim3(256), 0, st, gy, signbits, x, x2, part, nps, U, p.step, p.per);
    else hipLaunchKernelGGL((se_bwd_reduce_kernel<false, T>), dim3(p.G, B, p.gz), dim3(256), 0, st, gy, signbits, x, x2, part, nps, U, p.step, p.per);
    LOANS_LAUNCH_CHECK();
    hipLaunchKernelGGL((se_fold_kernel<double>), dim3(grid_for((int64_t)B * NS * C, 256, 1 << 30)), dim3(256), 0, st, part, G0, G1, G2,
                       B, p.G, NS, C);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

template <typename T>
static int bn_bwd_apply_gate_impl(const void* gy_, const uint8_t* signbits, const float* gate, const float* t, const void* x_,
                                  const float* k1, const float* k2, const float* k3, void* gx_, const void* x2_, const float* k1b,
                                  const float* k2b, const float* k3b, void* gx2_, int32_t B, int64_t P, int32_t C, void* stream) {
    const T *gy = static_cast<const T*>(gy_), *x = static_cast<const T*>(x_), *x2 = static_cast<const T*>(x2_);
    T *gx = static_cast<T*>(gx_), *gx2 = static_cast<T*>(gx2_);
    if (!gy || !signbits || !gate || !t || !x || !k1 || !k2 || !k3 || !gx) return LOANS_EINVAL;
    if (x2 && (!k1b || !k2b || !k3b || !gx2)) return LOANS_EINVAL;
    if (mis16(gy) || mis16(x) || mis16(gx) || mis16(x2) || mis16(gx2) || mis16(gate) || mis16(t) || mis16(k1) || mis16(k2) ||
        mis16(k3) || mis16(k1b) || mis16(k2b) || mis16(k3b) || ((uintptr_t)signbits & 1))
        return LOANS_EINVAL;
    int U;
    if (int rc = se_check<T>(B, P, C, &U)) return rc;
    const SePlan p = se_plan(B, P, U);
    const int64_t nps = P * U;
    const bool nt = slab_nt((int64_t)B * nps * 16);
    hipStream_t st = as_stream(stream);
#define LAUNCH_PG_(D, N_) hipLaunchKernelGGL((bn_bwd_apply_gate_kernel<D, N_, T>), dim3(p.G, B, p.gz), dim3(256), 0, st, gy, signbits, gate, t, x, k1, k2, k3, gx, x2, k1b, k2b, k3b, gx2, nps, U, p.step, p.per)
#define LAUNCH_PG(D) do { if (nt) LAUNCH_PG_(D, true); else LAUNCH_PG_(D, false); } while (0)
    if (x2) LAUNCH_PG(true); else LAUNCH_PG(false);
#undef LAUNCH_PG
#undef LAUNCH_PG_
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

}  // namespace

extern "C" int loans_se_slabs(int32_t B, int64_t rows_per_sample, int32_t C, int32_t elt_bytes) {
    if (elt_bytes == 4) return se_slabs_impl<float>(B, rows_per_sample, C);
    if (elt_bytes == 2) return se_slabs_impl<__bf16>(B, rows_per_sample, C);
    return LOANS_EINVAL;
}

extern "C" int loans_se_squeeze_f32(const float* x, float* S, float* partial, int32_t B, int64_t rows_per_sample, int32_t C,
                                    void* stream) {
    return se_squeeze_impl<float>(x, S, partial, B, rows_per_sample, C, stream);
}

extern "C" int loans_se_squeeze_bf16(const void* x, float* S, float* partial, int32_t B, int64_t rows_per_sample, int32_t C,
                                     void* stream) {
    return se_squeeze_impl<__bf16>(x, S, partial, B, rows_per_sample, C, stream);
}

extern "C" int loans_se_excite_fwd_f32(const float* S, const float* scale, const float* shift, const float* W1, const float* b1,
                                       const float* W2, const float* b2, float* s, float* h, float* q, int32_t B,
                                       int64_t rows_per_sample, int32_t C, int32_t hidden, void* stream) {
    if (!S || !scale || !shift || !W1 || !b1 || !W2 || !b2 || !s || !h || !q || mis16(W1) || mis16(W2)) return LOANS_EINVAL;
    if (B <= 0 || rows_per_sample <= 0 || !se_hidden_ok(C, hidden)) return LOANS_EINVAL;
    hipLaunchKernelGGL(se_excite_fwd_kernel, dim3(B), dim3(256), 0, as_stream(stream), S, scale, shift, W1, b1, W2, b2, s, h, q, C,
                       hidden, (float)(1.0 / (double)rows_per_sample));
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_bn_apply_gate_f32(const float* x, const float* scale, const float* shift, const float* x2, const float* scale2,
                                       const float* shift2, const float* s, float* y, uint8_t* signbits, int32_t B,
                                       int64_t rows_per_sample, int32_t C, int32_t mode, void* stream) {
    return bn_apply_gate_impl<float>(x, scale, shift, x2, scale2, shift2, s, y, signbits, B, rows_per_sample, C, mode, stream);
}

extern "C" int loans_bn_apply_gate_bf16(const void* x, const float* scale, const float* shift, const void* x2, const float* scale2,
                                        const float* shift2, const float* s, void* y, uint8_t* signbits, int32_t B,
                                        int64_t rows_per_sample, int32_t C, int32_t mode, void* stream) {
    return bn_apply_gate_impl<__bf16>(x, scale, shift, x2, scale2, shift2, s, y, signbits, B, rows_per_sample, C, mode, stream);
}

extern "C" int loans_se_bwd_reduce_f32(const float* gy, const uint8_t* signbits, const float* x, const float* x2, float* G0, float* G1,
                                       float* G2, double* partial, int32_t B, int64_t rows_per_sample, int32_t C, void* stream) {
    return se_bwd_reduce_impl<float>(gy, signbits, x, x2, G0, G1, G2, partial, B, rows_per_sample, C, stream);
}

extern "C" int loans_se_bwd_reduce_bf16(const void* gy, const uint8_t* signbits, const void* x, const void* x2, float* G0, float* G1,
                                        float* G2, double* partial, int32_t B, int64_t rows_per_sample, int32_t C, void* stream) {
    return se_bwd_reduce_impl<__bf16>(gy, signbits, x, x2, G0, G1, G2, partial, B, rows_per_sample, C, stream);
}

extern "C" int loans_se_excite_bwd_f32(const float* G0, const float* G1, const float* G2, const float* S, const float* scale,
                                       const float* shift, const float* mean, const float* rstd, const float* mean2,
                                       const float* rstd2, const float* s, const float* h, const float* q, const float* W1,
                                       const float* W2, float* t, float* da2, float* dh, double* u, float* gW1, float* gb1, float* gW2,
                                       float* gb2, double* sums, int32_t B, int64_t rows_per_sample, int32_t C, int32_t hidden,
                                       void* stream) {
    if (!G0 || !G1 || !S || !scale || !shift || !mean || !rstd || !s || !h || !q || !W1 || !W2 || !t || !da2 || !dh || !u || !gW1 ||
        !gb1 || !gW2 || !gb2 || !sums || (G2 && (!mean2 || !rstd2)) || ((uintptr_t)u & 7) || ((uintptr_t)sums & 7))
        return LOANS_EINVAL;
    if (B <= 0 || rows_per_sample <= 0 || !se_hidden_ok(C, hidden)) return LOANS_EINVAL;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(se_excite_bwd_kernel, dim3(B), dim3(256), 0, st, G0, G1, S, scale, shift, mean, s, h, W1, W2, t, da2, dh, u, C,
                       hidden, (float)(1.0 / (double)rows_per_sample), (float)rows_per_sample);
    LOANS_LAUNCH_CHECK();
    const int64_t n = 2 * (int64_t)C * hidden + C + hidden + (G2 ? 4 : 2) * (int64_t)C;
    hipLaunchKernelGGL(se_excite_bwd_fold_kernel, dim3(grid_for(n, 256, 1 << 30)), dim3(256), 0, st, da2, dh, h, q, u, rstd, G0, G2,
                       mean2, rstd2, gW1, gb1, gW2, gb2, sums, B, C, hidden);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_bn_bwd_apply_gate_f32(const float* gy, const uint8_t* signbits, const float* s, const float* t, const float* x,
                                           const float* k1, const float* k2, const float* k3, float* gx, const float* x2,
                                           const float* k1b, const float* k2b, const float* k3b, float* gx2, int32_t B,
                                           int64_t rows_per_sample, int32_t C, void* stream) {
    return bn_bwd_apply_gate_impl<float>(gy, signbits, s, t, x, k1, k2, k3, gx, x2, k1b, k2b, k3b, gx2, B, rows_per_sample, C, stream);
}

extern "C" int loans_bn_bwd_apply_gate_bf16(const void* gy, const uint8_t* signbits, const float* s, const float* t, const void* x,
                                            const float* k1, const float* k2, const float* k3, void* gx, const void* x2,
                                            const float* k1b, const float* k2b, const float* k3b, void* gx2, int32_t B,
                                            int64_t rows_per_sample, int32_t C, void* stream) {
    return bn_bwd_apply_gate_impl<__bf16>(gy, signbits, s, t, x, k1, k2, k3, gx, x2, k1b, k2b, k3b, gx2, B, rows_per_sample, C, stream);
}
