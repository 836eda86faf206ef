// The ImageNet classification head: a wide Linear layer (9 .. 2^16 outputs) in three directions on the fp32 matrix cores
// (v_mfma_f32_32x32x2_f32), and softmax cross-entropy with top-1 accuracy in one pass over the logits (and its label-smoothed
// form with a top-k hit, and the two-label form of a mixup / CutMix batch), and the evaluation form that writes no gradient and
// adds the batch to running sums in double.
// No atomics anywhere in this file: every output element is owned by one lane (GEMM) or one block (loss rows) and is summed
// in an order that depends on the shape alone, so two launches on the same inputs give the same bits.
#include "common.h"

namespace {

// ---- small GEMM ------------------------------------------------------------------------------------------------------------
// out[m][c] (+)= sum_r A(m, r) * Bm(r, c) (+ bias[c]),   m < M, c < C, r < R
//   A(m, r)  = A[m * lda + r]  (A_RC: r contiguous)   or  A[r * lda + m]   (m contiguous)
//   Bm(r, c) = Bm[c * ldb + r] (B_RC: r contiguous)   or  Bm[r * ldb + c]  (c contiguous)
// Block = 4 waves = a 64 x 64 tile of `out`, one 32 x 32 accumulator per wave; the reduction runs in chunks of GK through LDS
// images [r][m] and [r][c] (what one MFMA reads -- 32 consecutive floats per half wave -- is conflict free).  Rows, columns
// and reduction indices past the edge are staged as zeros: fma(0, 0, acc) leaves acc bit for bit, so a ragged tile sums
// exactly its own terms, in increasing r.  The MFMA is a k-ordered chain of fp32 fmaf: acc = fma(a_r, b_r, acc), r = 0 .. R-1.
constexpr int GT = 64;          // tile edge
constexpr int GK = 16;          // reduction chunk
constexpr int GLD = GT + 4;     // LDS row pitch (floats)

template <bool RC>
__device__ __forceinline__ void stage_tile(const float* __restrict__ src, int ld, int e0, int E, int r0, int R,
                                           float (*dst)[GLD], int tid) {
    if (RC) {           // src[e * ld + r]: 16 consecutive threads walk r
        const int r = tid & (GK - 1), gr = r0 + r;
#pragma unroll
        for (int i = 0; i < GT / 16; ++i) {
            const int e = (tid >> 4) + 16 * i, ge = e0 + e;
            dst[r][e] = (ge < E && gr < R) ? src[(int64_t)ge * ld + gr] : 0.f;
        }
    } else {            // src[r * ld + e]: 64 consecutive threads walk e
        const int e = tid & (GT - 1), ge = e0 + e;
#pragma unroll
        for (int i = 0; i < GK / 4; ++i) {
            const int r = (tid >> 6) + 4 * i, gr = r0 + r;
            dst[r][e] = (ge < E && gr < R) ? src[(int64_t)gr * ld + ge] : 0.f;
        }
    }
}

template <bool A_RC, bool B_RC>
__global__ __launch_bounds__(256) void gemm_tile_kernel(const float* __restrict__ A, int lda, const float* __restrict__ Bm, int ldb,
                                                        const float* __restrict__ bias, float* __restrict__ out, int ldo,
                                                        int M, int C, int R, int accumulate) {
    __shared__ float As[GK][GLD];
    __shared__ float Bs[GK][GLD];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * GT, c0 = blockIdx.x * GT;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    for (int r0 = 0; r0 < R; r0 += GK) {
        stage_tile<A_RC>(A, lda, m0, M, r0, R, As, tid);
        stage_tile<B_RC>(Bm, ldb, c0, C, r0, R, Bs, tid);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GK; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + h][wm * 32 + r], Bs[kk + h][wn * 32 + r], acc, 0, 0, 0);
        __syncthreads();
    }
    const int c = c0 + wn * 32 + r;
    if (c >= C) return;
    const float bv = bias ? bias[c] : 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int m = m0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (m < M) {
            float* o = out + (int64_t)m * ldo + c;
            float v = acc[e] + bv;
            if (accumulate) v += *o;
            *o = v;
        }
    }
}

// gb[n] += sum_b gy[b][n], b increasing: one thread per column
__global__ __launch_bounds__(256) void colsum_ordered_kernel(const float* __restrict__ gy, float* __restrict__ gb, int B, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += gy[(int64_t)b * N + n];
    gb[n] += s;
}

// ---- softmax cross-entropy -------------------------------------------------------------------------------------------------
// 256-thread block sum in a fixed tree: 6 butterfly levels inside each wave, then (w0 + w1) + (w2 + w3); valid in every thread
__device__ __forceinline__ float block_sum_256(float v, float* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__device__ __forceinline__ int block_count_256(int v, int* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// ---- one row of logits, shared by the three row kernels below (256 threads, the row kept in LDS) -----------------------------
// stage zr[0 .. N) into row[] (STAGE; without it the row is only read) and leave its maximum and the first index that holds it
// in every thread
template <bool STAGE = true>
__device__ __forceinline__ void row_stage_argmax(const float* __restrict__ zr, float* row, int N, float* shf, int* shi,
                                                 float& m, int& am) {
    const int tid = threadIdx.x;
    m = -INFINITY;
    am = 0x7fffffff;
    for (int i = tid; i < N; i += 256) {
        const float v = zr[i];
        if (STAGE) row[i] = v;
        if (v > m || am == 0x7fffffff) { m = v; am = i; }       // strictly greater: the earlier index stays on a tie
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        const int oa = __shfl_xor(am, o, 64);
        if (oa != 0x7fffffff && (am == 0x7fffffff || om > m || (om == m && oa < am))) { m = om; am = oa; }
    }
    __syncthreads();
    if ((tid & 63) == 0) { shf[tid >> 6] = m; shi[tid >> 6] = am; }
    __syncthreads();
    m = shf[0]; am = shi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const float om = shf[w];
        const int oa = shi[w];
        if (oa != 0x7fffffff && (am == 0x7fffffff || om > m || (om == m && oa < am))) { m = om; am = oa; }
    }
}

// S = sum exp(row - m), in the fixed tree
__device__ __forceinline__ float row_sum_exp(const float* row, int N, float m, float* shf) {
    float s = 0.f;
    for (int i = threadIdx.x; i < N; i += 256) s += expf(row[i] - m);
    return block_sum_256(s, shf);
}

// #{ j : row_j > zt or (row_j == zt and j < label) }: the label's place in the row, 0 = first
__device__ __forceinline__ int row_rank(const float* row, int N, int label, float zt, int* shi) {
    int ahead = 0;
    for (int i = threadIdx.x; i < N; i += 256) {
        const float v = row[i];
        ahead += (v > zt) || (v == zt && i < label);
    }
    return block_count_256(ahead, shi);
}

// one block per row; the row is read from memory once and kept in LDS (dynamic, N floats)
//   m = max z, first index wins a tie;  S = sum exp(z - m);  lse = m + log S;  loss = lse - z[t]
//   gz = (exp(z - m) / S - onehot) / count        count = max(#rows with a label in [0, N), 1)
// rows whose label is outside [0, N) (-1 = ignore_label; anything else out of range is treated the same way): loss 0, gz 0.
__global__ __launch_bounds__(256) void softmax_xent_rows_kernel(const float* __restrict__ z, const int* __restrict__ t,
                                                                float* __restrict__ gz, float* __restrict__ row_loss,
                                                                float* __restrict__ row_hit, int B, int N) {
    extern __shared__ __attribute__((aligned(16))) float row[];
    __shared__ float shf[4];
    __shared__ int shi[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float* zr = z + (int64_t)b * N;
    float* gr = gz + (int64_t)b * N;

    int valid = 0;
    for (int i = tid; i < B; i += 256) valid += (unsigned)t[i] < (unsigned)N;
    const int count = max(block_count_256(valid, shi), 1);

    float m;
    int am;
    row_stage_argmax(zr, row, N, shf, shi, m, am);

    const int label = t[b];
    if (tid == 0) row_hit[b] = (am == label) ? 1.f : 0.f;
    if ((unsigned)label >= (unsigned)N) {       // ignored row (uniform per block)
        for (int i = tid; i < N; i += 256) gr[i] = 0.f;
        if (tid == 0) row_loss[b] = 0.f;
        return;
    }
    const float S = row_sum_exp(row, N, m, shf);
    if (tid == 0) row_loss[b] = (m + logf(S)) - row[label];
    const float fc = (float)count;
    for (int i = tid; i < N; i += 256) {
        const float p = expf(row[i] - m) / S;
        gr[i] = (p - (i == label ? 1.f : 0.f)) / fc;
    }
}

// out[0] = (sum_b row_loss[b]) / count ; out[1] = (sum_b row_hit[b]) / B   -- one block, the same fixed tree
__global__ __launch_bounds__(256) void softmax_xent_reduce_kernel(const float* __restrict__ row_loss, const float* __restrict__ row_hit,
                                                                  const int* __restrict__ t, float* __restrict__ out, int B, int N) {
    __shared__ float shf[4];
    __shared__ int shi[4];
    const int tid = threadIdx.x;
    int valid = 0;
    float l = 0.f, a = 0.f;
    for (int i = tid; i < B; i += 256) {
        valid += (unsigned)t[i] < (unsigned)N;
        l += row_loss[i];
        a += row_hit[i];
    }
    const int count = max(block_count_256(valid, shi), 1);
    const float L = block_sum_256(l, shf);
    const float A = block_sum_256(a, shf);
    if (tid == 0) { out[0] = L / (float)count; out[1] = A / (float)B; }
}

// The label-smoothed form with a top-k hit beside the top-1 one (loans_softmax_xent_ls_fwd_f32).  Target distribution
//   q = (1 - eps) onehot(t) + eps / N          (uniform over all N classes: torch's label_smoothing)
//   loss = lse - (1 - eps) z_t - eps mean(z),  gz = (softmax(z) - q) / count
//   hitk = #{ j : z_j > z_t or (z_j == z_t and j < t) } < k        (k = 1: the top-1 hit, first index wins a tie)
// mean(z) and the rank are two more block reductions over the LDS row.  eps == 0 (uniform over the launch) takes the expressions
// of softmax_xent_rows_kernel, so loss, gz and hit carry its bits.
struct XentLs { float eps, omeps, q_off, q_on; int k; };        // q_off = eps / N, q_on = (1 - eps) + eps / N

__global__ __launch_bounds__(256) void softmax_xent_ls_rows_kernel(const float* __restrict__ z, const int* __restrict__ t,
                                                                   float* __restrict__ gz, float* __restrict__ row_loss,
                                                                   float* __restrict__ row_hit, float* __restrict__ row_hitk,
                                                                   int B, int N, XentLs ls) {
    extern __shared__ __attribute__((aligned(16))) float row[];
    __shared__ float shf[4];
    __shared__ int shi[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float* zr = z + (int64_t)b * N;
    float* gr = gz + (int64_t)b * N;

    int valid = 0;
    for (int i = tid; i < B; i += 256) valid += (unsigned)t[i] < (unsigned)N;
    const int count = max(block_count_256(valid, shi), 1);

    float m;
    int am;
    row_stage_argmax(zr, row, N, shf, shi, m, am);

    const int label = t[b];
    if (tid == 0) row_hit[b] = (am == label) ? 1.f : 0.f;
    if ((unsigned)label >= (unsigned)N) {       // ignored row (uniform per block)
        for (int i = tid; i < N; i += 256) gr[i] = 0.f;
        if (tid == 0) { row_loss[b] = 0.f; row_hitk[b] = 0.f; }
        return;
    }
    const float zt = row[label];
    const int rank = row_rank(row, N, label, zt, shi);
    if (tid == 0) row_hitk[b] = (rank < ls.k) ? 1.f : 0.f;

    const float S = row_sum_exp(row, N, m, shf);
    const float fc = (float)count;
    if (ls.eps == 0.f) {
        if (tid == 0) row_loss[b] = (m + logf(S)) - zt;
        for (int i = tid; i < N; i += 256) {
            const float p = expf(row[i] - m) / S;
            gr[i] = (p - (i == label ? 1.f : 0.f)) / fc;
        }
        return;
    }
    float zs = 0.f;
    for (int i = tid; i < N; i += 256) zs += row[i];
    const float mean = block_sum_256(zs, shf) / (float)N;
    if (tid == 0) row_loss[b] = ((m + logf(S)) - ls.omeps * zt) - ls.eps * mean;
    for (int i = tid; i < N; i += 256) {
        const float p = expf(row[i] - m) / S;
        gr[i] = (p - (i == label ? ls.q_on : ls.q_off)) / fc;
    }
}

// out[0] = (sum_b row_loss[b]) / count ; out[1] = (sum_b row_hit[b]) / B ; out[2] = (sum_b row_hitk[b]) / B
__global__ __launch_bounds__(256) void softmax_xent_ls_reduce_kernel(const float* __restrict__ row_loss, const float* __restrict__ row_hit,
                                                                     const float* __restrict__ row_hitk, const int* __restrict__ t,
                                                                     float* __restrict__ out, int B, int N) {
    __shared__ float shf[4];
    __shared__ int shi[4];
    const int tid = threadIdx.x;
    int valid = 0;
    float l = 0.f, a = 0.f, ak = 0.f;
    for (int i = tid; i < B; i += 256) {
        valid += (unsigned)t[i] < (unsigned)N;
        l += row_loss[i];
        a += row_hit[i];
        ak += row_hitk[i];
    }
    const int count = max(block_count_256(valid, shi), 1);
    const float L = block_sum_256(l, shf);
    const float A = block_sum_256(a, shf);
    const float AK = block_sum_256(ak, shf);
    if (tid == 0) { out[0] = L / (float)count; out[1] = A / (float)B; out[2] = AK / (float)B; }
}

// The two-label form (loans_softmax_xent_mix_fwd_f32: the target of a mixup / CutMix batch).  With w_i = lam [i == ta] + oml [i == tb]
// (ta == tb: the sum of the two weights on that class)
//   q = (1 - eps) w + eps / N,   loss = lse - (1 - eps) (lam z_ta + oml z_tb) - eps mean(z),   gz = (softmax(z) - q) / count
// A row counts when BOTH labels lie in [0, N); hit and rank are taken against the dominant label (ta if lam >= oml, else tb).
// The products are plain C++: the compiler may contract a multiply-add, which removes a rounding and adds none.  This kernel
// never sees the weights (1, 0) or (0, 1): the launcher hands those to softmax_xent_ls_rows_kernel on the one label that counts.
struct XentMix { XentLs ls; float lam, oml; };

__global__ __launch_bounds__(256) void softmax_xent_mix_rows_kernel(const float* __restrict__ z, const int* __restrict__ ta,
                                                                    const int* __restrict__ tb, float* __restrict__ gz,
                                                                    float* __restrict__ row_loss, float* __restrict__ row_hit,
                                                                    float* __restrict__ row_hitk, int B, int N, XentMix mx) {
    extern __shared__ __attribute__((aligned(16))) float row[];
    __shared__ float shf[4];
    __shared__ int shi[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float* zr = z + (int64_t)b * N;
    float* gr = gz + (int64_t)b * N;

    int valid = 0;
    for (int i = tid; i < B; i += 256) valid += ((unsigned)ta[i] < (unsigned)N) & ((unsigned)tb[i] < (unsigned)N);
    const int count = max(block_count_256(valid, shi), 1);

    float m;
    int am;
    row_stage_argmax(zr, row, N, shf, shi, m, am);

    const int la = ta[b], lb = tb[b];
    if ((unsigned)la >= (unsigned)N || (unsigned)lb >= (unsigned)N) {       // ignored row (uniform per block)
        for (int i = tid; i < N; i += 256) gr[i] = 0.f;
        if (tid == 0) { row_loss[b] = 0.f; row_hit[b] = 0.f; row_hitk[b] = 0.f; }
        return;
    }
    const int label = mx.lam >= mx.oml ? la : lb;
    if (tid == 0) row_hit[b] = (am == label) ? 1.f : 0.f;
    const int rank = row_rank(row, N, label, row[label], shi);
    if (tid == 0) row_hitk[b] = (rank < mx.ls.k) ? 1.f : 0.f;

    const float zmix = mx.lam * row[la] + mx.oml * row[lb];
    const float S = row_sum_exp(row, N, m, shf);
    const float fc = (float)count;
    if (mx.ls.eps == 0.f) {
        if (tid == 0) row_loss[b] = (m + logf(S)) - zmix;
    } else {
        float zs = 0.f;
        for (int i = tid; i < N; i += 256) zs += row[i];
        const float mean = block_sum_256(zs, shf) / (float)N;
        if (tid == 0) row_loss[b] = ((m + logf(S)) - mx.ls.omeps * zmix) - mx.ls.eps * mean;
    }
    // (eps == 0: omeps = 1 and q_off = 0, so q is w itself)
    for (int i = tid; i < N; i += 256) {
        const float p = expf(row[i] - m) / S;
        const float w = (i == la ? mx.lam : 0.f) + (i == lb ? mx.oml : 0.f);
        gr[i] = (p - (mx.ls.omeps * w + mx.ls.q_off)) / fc;
    }
}

// softmax_xent_ls_reduce_kernel with the two-label count
__global__ __launch_bounds__(256) void softmax_xent_mix_reduce_kernel(const float* __restrict__ row_loss, const float* __restrict__ row_hit,
                                                                      const float* __restrict__ row_hitk, const int* __restrict__ ta,
                                                                      const int* __restrict__ tb, float* __restrict__ out, int B, int N) {
    __shared__ float shf[4];
    __shared__ int shi[4];
    const int tid = threadIdx.x;
    int valid = 0;
    float l = 0.f, a = 0.f, ak = 0.f;
    for (int i = tid; i < B; i += 256) {
        valid += ((unsigned)ta[i] < (unsigned)N) & ((unsigned)tb[i] < (unsigned)N);
        l += row_loss[i];
        a += row_hit[i];
        ak += row_hitk[i];
    }
    const int count = max(block_count_256(valid, shi), 1);
    const float L = block_sum_256(l, shf);
    const float A = block_sum_256(a, shf);
    const float AK = block_sum_256(ak, shf);
    if (tid == 0) { out[0] = L / (float)count; out[1] = A / (float)B; out[2] = AK / (float)B; }
}

// Per-class sigmoid binary cross-entropy against the two-label target (loans_sigmoid_bce_fwd_f32: the loss of timm's A1 - A3
// procedures).  The target is the mix kernel's, q = (1 - eps) w + eps / N with w_i = lam [i == ta] + oml [i == tb], made 0 / 1 by
// the strict comparison q > thresh where a threshold is given (thresh < 0: none).  Per element, with e = expf(-|z|) in (0, 1]:
//   l = max(z, 0) - z q + log1pf(e)                    never exp(z) itself: finite for every finite z
//   s = z >= 0 ? 1 / (1 + e) : e / (1 + e)             the sigmoid
//   row_loss = sum_i l_i,   gz = (s - q) / denom,   denom = count * N (the mean over classes) or count (sum_classes)
// A row counts when BOTH labels lie in [0, N); hit and rank are those of the softmax kernels (the sigmoid is monotone), against
// the dominant label.  The launcher hands a one-label call the same array twice, so the weights (1, 0) and (0, 1) need no code
// of their own: w is lam + oml = 1 on the one label, and the array of weight zero is never seen.  denom is one fp32 rounding of
// the integer count * N (at most 2^29), formed the same way in the reduce kernel.
struct SigmoidBce { float lam, oml, omeps, q_off, thresh; int k, sum_classes; };

__device__ __forceinline__ float bce_denom(int count, int N, int sum_classes) { return (float)(sum_classes ? count : count * N); }

__global__ __launch_bounds__(256) void sigmoid_bce_rows_kernel(const float* __restrict__ z, const int* __restrict__ ta,
                                                               const int* __restrict__ tb, float* __restrict__ gz,
                                                               float* __restrict__ row_loss, float* __restrict__ row_hit,
                                                               float* __restrict__ row_hitk, int B, int N, SigmoidBce bc) {
    extern __shared__ __attribute__((aligned(16))) float row[];
    __shared__ float shf[4];
    __shared__ int shi[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float* zr = z + (int64_t)b * N;
    float* gr = gz + (int64_t)b * N;

    int valid = 0;
    for (int i = tid; i < B; i += 256) valid += ((unsigned)ta[i] < (unsigned)N) & ((unsigned)tb[i] < (unsigned)N);
    const int count = max(block_count_256(valid, shi), 1);

    float m;
    int am;
    row_stage_argmax(zr, row, N, shf, shi, m, am);

    const int la = ta[b], lb = tb[b];
    if ((unsigned)la >= (unsigned)N || (unsigned)lb >= (unsigned)N) {       // ignored row (uniform per block)
        for (int i = tid; i < N; i += 256) gr[i] = 0.f;
        if (tid == 0) { row_loss[b] = 0.f; row_hit[b] = 0.f; row_hitk[b] = 0.f; }
        return;
    }
    const int label = bc.lam >= bc.oml ? la : lb;
    if (tid == 0) row_hit[b] = (am == label) ? 1.f : 0.f;
    const int rank = row_rank(row, N, label, row[label], shi);
    if (tid == 0) row_hitk[b] = (rank < bc.k) ? 1.f : 0.f;

    const float denom = bce_denom(count, N, bc.sum_classes);
    float ls = 0.f;
    for (int i = tid; i < N; i += 256) {
        const float v = row[i];
        const float w = (i == la ? bc.lam : 0.f) + (i == lb ? bc.oml : 0.f);
        float q = bc.omeps * w + bc.q_off;
        if (bc.thresh >= 0.f) q = q > bc.thresh ? 1.f : 0.f;
        const float e = expf(-fabsf(v));
        ls += (fmaxf(v, 0.f) - v * q) + log1pf(e);
        const float s = (v >= 0.f ? 1.f : e) / (1.f + e);
        gr[i] = (s - q) / denom;
    }
    const float L = block_sum_256(ls, shf);
    if (tid == 0) row_loss[b] = L;
}

// out[0] = (sum_b row_loss[b]) / denom ; out[1] = (sum_b row_hit[b]) / B ; out[2] = (sum_b row_hitk[b]) / B
__global__ __launch_bounds__(256) void sigmoid_bce_reduce_kernel(const float* __restrict__ row_loss, const float* __restrict__ row_hit,
                                                                 const float* __restrict__ row_hitk, const int* __restrict__ ta,
                                                                 const int* __restrict__ tb, float* __restrict__ out, int B, int N,
                                                                 int sum_classes) {
    __shared__ float shf[4];
    __shared__ int shi[4];
    const int tid = threadIdx.x;
    int valid = 0;
    float l = 0.f, a = 0.f, ak = 0.f;
    for (int i = tid; i < B; i += 256) {
        valid += ((unsigned)ta[i] < (unsigned)N) & ((unsigned)tb[i] < (unsigned)N);
        l += row_loss[i];
        a += row_hit[i];
        ak += row_hitk[i];
    }
    const int count = max(block_count_256(valid, shi), 1);
    const float L = block_sum_256(l, shf);
    const float A = block_sum_256(a, shf);
    const float AK = block_sum_256(ak, shf);
    if (tid == 0) { out[0] = L / bce_denom(count, N, sum_classes); out[1] = A / (float)B; out[2] = AK / (float)B; }
}

// Knowledge distillation against a frozen teacher's logits (loans_softmax_distill_fwd_f32; Hinton's convention, torch's
// kl_div(log_softmax(z / T), softmax(zt / T), 'batchmean') T^2 beside the mix kernel's hard loss).  With invT = fl(1 / T) from
// the host and the ROUNDED products zs = fl(z invT), zts = fl(zt invT)  (mul_rounded: never contracted into the subtraction that
// follows, so the scaled logits are the same numbers wherever they are used, and the maximum of a scaled row is the scaled
// maximum, rounding being monotone):
//   y = softmax(z), s = softmax(zs), p = softmax(zts),   hard = the mix kernel's row loss, by its expressions
//   kl = sum_i p_i (((zts_i - mts) - log St) - ((zs_i - ms) - log Ss))        shifted logits and lse, never log(p): finite for
//                                                                              every finite pair; p_i == 0 gives 0 * finite = 0
//   row_kl = T2 kl,   row_loss = oma hard + alpha row_kl,   gz = (oma (y - q) + aT (s - p)) / count
// oma = fl(1 - alpha), alpha, T2 = fl(T^2), aT = fl(alpha T) are rounded once on the host.  Every other multiply-add is plain C++:
// a contraction removes the rounding of a product and adds none, and the bound of tests/imagenet_distill/reference.py covers both
// codes (as for the BCE kernel).  The student row is staged in LDS (N floats, as in every kernel here); the teacher row is read
// from memory three times -- argmax, sum, gradient -- 4 KB at N = 1000 that stays in the vector cache, which keeps LDS at 32 KB for
// N = 8192 and the occupancy of the siblings.  Three sums (S, Ss, St) and the mean come from ONE pass over the LDS row, kl from
// the second.  Bound by launch latency and its eight block reductions, not by bandwidth: 3 MB move at B = 256, N = 1000.
// A row counts when both labels lie in [0, N); the launcher hands a one-label call the same array twice (as for the BCE kernel).
// row_thit: the teacher's argmax (first index on a tie, on zt itself) against the dominant label.
struct Distill { XentMix mx; float invT, oma, alpha, T2, aT; };

__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

__global__ __launch_bounds__(256) void softmax_distill_rows_kernel(const float* __restrict__ z, const float* __restrict__ zt,
                                                                   const int* __restrict__ ta, const int* __restrict__ tb,
                                                                   float* __restrict__ gz, float* __restrict__ row_loss,
                                                                   float* __restrict__ row_hit, float* __restrict__ row_hitk,
                                                                   float* __restrict__ row_kl, float* __restrict__ row_thit,
                                                                   int B, int N, Distill ds) {
    extern __shared__ __attribute__((aligned(16))) float row[];
    __shared__ float shf[4];
    __shared__ int shi[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float* zr = z + (int64_t)b * N;
    const float* tr = zt + (int64_t)b * N;
    float* gr = gz + (int64_t)b * N;
    const XentMix& mx = ds.mx;

    int valid = 0;
    for (int i = tid; i < B; i += 256) valid += ((unsigned)ta[i] < (unsigned)N) & ((unsigned)tb[i] < (unsigned)N);
    const int count = max(block_count_256(valid, shi), 1);

    const int la = ta[b], lb = tb[b];
    if ((unsigned)la >= (unsigned)N || (unsigned)lb >= (unsigned)N) {       // ignored row (uniform per block)
        for (int i = tid; i < N; i += 256) gr[i] = 0.f;
        if (tid == 0) { row_loss[b] = 0.f; row_hit[b] = 0.f; row_hitk[b] = 0.f; row_kl[b] = 0.f; row_thit[b] = 0.f; }
        return;
    }
    float m, mt;
    int am, amt;
    row_stage_argmax(zr, row, N, shf, shi, m, am);
    row_stage_argmax<false>(tr, nullptr, N, shf, shi, mt, amt);

    const int label = mx.lam >= mx.oml ? la : lb;
    if (tid == 0) { row_hit[b] = (am == label) ? 1.f : 0.f; row_thit[b] = (amt == label) ? 1.f : 0.f; }
    const int rank = row_rank(row, N, label, row[label], shi);
    if (tid == 0) row_hitk[b] = (rank < mx.ls.k) ? 1.f : 0.f;

    const float ms = mul_rounded(m, ds.invT), mts = mul_rounded(mt, ds.invT);
    float s = 0.f, ss = 0.f, st = 0.f, zsum = 0.f;
    for (int i = tid; i < N; i += 256) {
        const float v = row[i];
        s += expf(v - m);
        ss += expf(mul_rounded(v, ds.invT) - ms);
        st += expf(mul_rounded(tr[i], ds.invT) - mts);
        zsum += v;
    }
    const float S = block_sum_256(s, shf);
    const float Ss = block_sum_256(ss, shf);
    const float St = block_sum_256(st, shf);
    const float zmix = mx.lam * row[la] + mx.oml * row[lb];
    float hard;
    if (mx.ls.eps == 0.f) {
        hard = (m + logf(S)) - zmix;
    } else {
        const float mean = block_sum_256(zsum, shf) / (float)N;
        hard = ((m + logf(S)) - mx.ls.omeps * zmix) - mx.ls.eps * mean;
    }
    const float Ls = logf(Ss), Lt = logf(St);
    const float fc = (float)count;
    float kl = 0.f;
    for (int i = tid; i < N; i += 256) {
        const float v = row[i];
        const float y = expf(v - m) / S;
        const float dz = mul_rounded(v, ds.invT) - ms;
        const float dt = mul_rounded(tr[i], ds.invT) - mts;
        const float sp = expf(dz) / Ss;
        const float p = expf(dt) / St;
        kl += p * ((dt - Lt) - (dz - Ls));
        const float w = (i == la ? mx.lam : 0.f) + (i == lb ? mx.oml : 0.f);
        const float h = y - (mx.ls.omeps * w + mx.ls.q_off);
        gr[i] = (ds.oma * h + ds.aT * (sp - p)) / fc;
    }
    const float KL = block_sum_256(kl, shf);
    if (tid == 0) {
        const float rk = ds.T2 * KL;
        row_kl[b] = rk;
        row_loss[b] = ds.oma * hard + ds.alpha * rk;
    }
}

// softmax_xent_mix_reduce_kernel with the two sums more: out[3] = (sum_b row_kl[b]) / count, out[4] = (sum_b row_thit[b]) / B
__global__ __launch_bounds__(256) void softmax_distill_reduce_kernel(const float* __restrict__ row_loss, const float* __restrict__ row_hit,
                                                                     const float* __restrict__ row_hitk, const float* __restrict__ row_kl,
                                                                     const float* __restrict__ row_thit, const int* __restrict__ ta,
                                                                     const int* __restrict__ tb, float* __restrict__ out, int B, int N) {
    __shared__ float shf[4];
    __shared__ int shi[4];
    const int tid = threadIdx.x;
    int valid = 0;
    float l = 0.f, a = 0.f, ak = 0.f, kl = 0.f, at = 0.f;
    for (int i = tid; i < B; i += 256) {
        valid += ((unsigned)ta[i] < (unsigned)N) & ((unsigned)tb[i] < (unsigned)N);
        l += row_loss[i];
        a += row_hit[i];
        ak += row_hitk[i];
        kl += row_kl[i];
        at += row_thit[i];
    }
    const int count = max(block_count_256(valid, shi), 1);
    const float L = block_sum_256(l, shf);
    const float A = block_sum_256(a, shf);
    const float AK = block_sum_256(ak, shf);
    const float KL = block_sum_256(kl, shf);
    const float AT = block_sum_256(at, shf);
    if (tid == 0) {
        out[0] = L / (float)count; out[1] = A / (float)B; out[2] = AK / (float)B;
        out[3] = KL / (float)count; out[4] = AT / (float)B;
    }
}

// alpha == 0: the mix entry has written everything else; the teacher's outputs are zeros
__global__ __launch_bounds__(256) void softmax_distill_zero_kernel(float* __restrict__ row_kl, float* __restrict__ row_thit,
                                                                   float* __restrict__ out, int B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B) { row_kl[i] = 0.f; row_thit[i] = 0.f; }
    if (i < 2) out[3 + i] = 0.f;
}

// Evaluation (loans_softmax_xent_eval_f32): the plain loss, the top-1 and the top-k hit of every row -- the eps == 0 expressions
// of softmax_xent_ls_rows_kernel on the same row code -- and no gradient.  rows: [0, B) loss, [B, 2B) hit, [2B, 3B) top-k hit.
__global__ __launch_bounds__(256) void softmax_xent_eval_rows_kernel(const float* __restrict__ z, const int* __restrict__ t,
                                                                     float* __restrict__ rows, int B, int N, int k) {
    extern __shared__ __attribute__((aligned(16))) float row[];
    __shared__ float shf[4];
    __shared__ int shi[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    float m;
    int am;
    row_stage_argmax(z + (int64_t)b * N, row, N, shf, shi, m, am);
    const int label = t[b];
    if ((unsigned)label >= (unsigned)N) {       // ignored row (uniform per block)
        if (tid == 0) { rows[b] = 0.f; rows[B + b] = 0.f; rows[2 * B + b] = 0.f; }
        return;
    }
    const float zt = row[label];
    const int rank = row_rank(row, N, label, zt, shi);
    const float S = row_sum_exp(row, N, m, shf);
    if (tid == 0) {
        rows[b] = (m + logf(S)) - zt;
        rows[B + b] = (am == label) ? 1.f : 0.f;
        rows[2 * B + b] = (rank < k) ? 1.f : 0.f;
    }
}

__device__ __forceinline__ double block_sum_256_d(double v, double* sh) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// acc[0] += sum row loss (in double, the fixed tree), acc[1] += hits, acc[2] += top-k hits, acc[3] += valid rows, acc[4] += B:
// one block, thread 0 alone touches acc
__global__ __launch_bounds__(256) void softmax_xent_eval_reduce_kernel(const float* __restrict__ rows, const int* __restrict__ t,
                                                                       double* __restrict__ acc, int B, int N) {
    __shared__ double shd[4];
    __shared__ int shi[4];
    const int tid = threadIdx.x;
    int valid = 0, h = 0, hk = 0;
    double l = 0.0;
    for (int i = tid; i < B; i += 256) {
        valid += (unsigned)t[i] < (unsigned)N;
        l += (double)rows[i];
        h += rows[B + i] != 0.f;
        hk += rows[2 * B + i] != 0.f;
    }
    const double L = block_sum_256_d(l, shd);
    const int H = block_count_256(h, shi);
    const int HK = block_count_256(hk, shi);
    const int V = block_count_256(valid, shi);
    if (tid == 0) {
        acc[0] += L;
        acc[1] += (double)H;
        acc[2] += (double)HK;
        acc[3] += (double)V;
        acc[4] += (double)B;
    }
}

__global__ __launch_bounds__(256) void scale_by_scalar_kernel(const float* __restrict__ x, const float* __restrict__ s,
                                                              float* __restrict__ y, int64_t n) {
    const float g = s[0];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) y[i] = x[i] * g;
}

constexpr int WIDE_MAX = 1 << 16;           // B, K, N of the wide Linear
constexpr int XENT_MAX_N = 1 << 13;         // one row of logits in LDS: 32 KB
constexpr int XENT_MAX_B = 1 << 16;

int wide_shape_ok(int32_t B, int32_t K, int32_t N) {
    if (B <= 0 || K < 4 || (K & 3) || N < 9) return LOANS_EINVAL;
    if (B > WIDE_MAX || K > WIDE_MAX || N > WIDE_MAX) return LOANS_ERANGE;
    if ((int64_t)B * K >= (1ll << 31) || (int64_t)N * K >= (1ll << 31) || (int64_t)B * N >= (1ll << 31)) return LOANS_ERANGE;
    return LOANS_OK;
}

dim3 tiles(int M, int C) { return dim3((C + GT - 1) / GT, (M + GT - 1) / GT); }

}  // namespace

extern "C" int loans_linear_wide_fwd_f32(const float* x, const float* W, const float* b, float* y, int32_t B, int32_t K,
                                         int32_t N, void* stream) {
    if (!x || !W || !y) return LOANS_EINVAL;
    if (int rc = wide_shape_ok(B, K, N)) return rc;
    hipLaunchKernelGGL((gemm_tile_kernel<true, true>), tiles(B, N), dim3(256), 0, as_stream(stream), x, K, W, K, b, y, N, B, N, K, 0);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_linear_wide_bwd_f32(const float* x, const float* W, const float* gy, float* gx, float* gW, float* gb,
                                         int32_t B, int32_t K, int32_t N, void* stream) {
    if (!gy) return LOANS_EINVAL;
    if ((gx && !W) || (gW && !x)) return LOANS_EINVAL;
    if (!gx && !gW && !gb) return LOANS_EINVAL;
    if (int rc = wide_shape_ok(B, K, N)) return rc;
    hipStream_t st = as_stream(stream);
    if (gx) {       // gx[b][k] = sum_n gy[b][n] W[n][k]
        hipLaunchKernelGGL((gemm_tile_kernel<true, false>), tiles(B, K), dim3(256), 0, st, gy, N, W, K, (const float*)nullptr, gx, K, B, K, N, 0);
        LOANS_LAUNCH_CHECK();
    }
    if (gW) {       // gW[n][k] += sum_b gy[b][n] x[b][k]
        hipLaunchKernelGGL((gemm_tile_kernel<false, false>), tiles(N, K), dim3(256), 0, st, gy, N, x, K, (const float*)nullptr, gW, K, N, K, B, 1);
        LOANS_LAUNCH_CHECK();
    }
    if (gb) {
        hipLaunchKernelGGL(colsum_ordered_kernel, dim3((N + 255) / 256), dim3(256), 0, st, gy, gb, B, N);
        LOANS_LAUNCH_CHECK();
    }
    return LOANS_OK;
}

extern "C" int loans_softmax_xent_fwd_f32(const float* z, const int32_t* t, float* gz, float* row_loss, float* row_hit,
                                          float* out, int32_t B, int32_t N, void* stream) {
    if (!z || !t || !gz || !row_loss || !row_hit || !out || B <= 0 || N <= 0) return LOANS_EINVAL;
    if (N > XENT_MAX_N || B > XENT_MAX_B) return LOANS_ERANGE;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(softmax_xent_rows_kernel, dim3(B), dim3(256), (size_t)N * sizeof(float), st, z, t, gz, row_loss, row_hit, B, N);
    LOANS_LAUNCH_CHECK();
    hipLaunchKernelGGL(softmax_xent_reduce_kernel, dim3(1), dim3(256), 0, st, row_loss, row_hit, t, out, B, N);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_softmax_xent_ls_fwd_f32(const float* z, const int32_t* t, float* gz, float* row_loss, float* row_hit,
                                             float* row_hitk, float* out, int32_t B, int32_t N, double eps, int32_t k,
                                             void* stream) {
    if (!z || !t || !gz || !row_loss || !row_hit || !row_hitk || !out || B <= 0 || N <= 0) return LOANS_EINVAL;
    if (!(eps >= 0.0 && eps < 1.0) || k < 1) return LOANS_EINVAL;
    if (N > XENT_MAX_N || B > XENT_MAX_B) return LOANS_ERANGE;
    XentLs ls;
    ls.eps = (float)eps; ls.omeps = (float)(1.0 - eps); ls.q_off = (float)(eps / N); ls.q_on = ls.omeps + ls.q_off; ls.k = k;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(softmax_xent_ls_rows_kernel, dim3(B), dim3(256), (size_t)N * sizeof(float), st, z, t, gz, row_loss, row_hit,
                       row_hitk, B, N, ls);
    LOANS_LAUNCH_CHECK();
    hipLaunchKernelGGL(softmax_xent_ls_reduce_kernel, dim3(1), dim3(256), 0, st, row_loss, row_hit, row_hitk, t, out, B, N);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_softmax_xent_mix_fwd_f32(const float* z, const int32_t* ta, const int32_t* tb, float lam, float oml,
                                              float* gz, float* row_loss, float* row_hit, float* row_hitk, float* out,
                                              int32_t B, int32_t N, double eps, int32_t k, void* stream) {
    if (!z || !ta || !tb || !gz || !row_loss || !row_hit || !row_hitk || !out || B <= 0 || N <= 0) return LOANS_EINVAL;
    if (!(eps >= 0.0 && eps < 1.0) || k < 1 || !__builtin_isfinite(lam) || !__builtin_isfinite(oml)) return LOANS_EINVAL;
    // one label per row: the label-smoothed kernels themselves on the label that carries the whole weight -- their bits; the
    // other label is not read
    if (lam == 1.f && oml == 0.f) return loans_softmax_xent_ls_fwd_f32(z, ta, gz, row_loss, row_hit, row_hitk, out, B, N, eps, k, stream);
    if (lam == 0.f && oml == 1.f) return loans_softmax_xent_ls_fwd_f32(z, tb, gz, row_loss, row_hit, row_hitk, out, B, N, eps, k, stream);
    if (N > XENT_MAX_N || B > XENT_MAX_B) return LOANS_ERANGE;
    XentMix mx;
    mx.ls.eps = (float)eps; mx.ls.omeps = (float)(1.0 - eps); mx.ls.q_off = (float)(eps / N); mx.ls.q_on = mx.ls.omeps + mx.ls.q_off;
    mx.ls.k = k; mx.lam = lam; mx.oml = oml;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(softmax_xent_mix_rows_kernel, dim3(B), dim3(256), (size_t)N * sizeof(float), st, z, ta, tb, gz, row_loss,
                       row_hit, row_hitk, B, N, mx);
    LOANS_LAUNCH_CHECK();
    hipLaunchKernelGGL(softmax_xent_mix_reduce_kernel, dim3(1), dim3(256), 0, st, row_loss, row_hit, row_hitk, ta, tb, out, B, N);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_sigmoid_bce_fwd_f32(const float* z, const int32_t* ta, const int32_t* tb, float lam, float oml, float* gz,
                                         float* row_loss, float* row_hit, float* row_hitk, float* out, int32_t B, int32_t N,
                                         double eps, int32_t k, float thresh, int32_t sum_classes, void* stream) {
    if (!tb) { tb = ta; lam = 1.f; oml = 0.f; }         // one label
    if (!z || !ta || !gz || !row_loss || !row_hit || !row_hitk || !out || B <= 0 || N <= 0) return LOANS_EINVAL;
    if (!(eps >= 0.0 && eps < 1.0) || k < 1 || !__builtin_isfinite(lam) || !__builtin_isfinite(oml)) return LOANS_EINVAL;
    if (!(thresh < 1.f)) return LOANS_EINVAL;           // (a NaN too)
    if (N > XENT_MAX_N || B > XENT_MAX_B) return LOANS_ERANGE;
    // one label per row: the array that carries the whole weight in both places, so the other one is not read
    if (lam == 1.f && oml == 0.f) tb = ta;
    if (lam == 0.f && oml == 1.f) ta = tb;
    SigmoidBce bc;
    bc.lam = lam; bc.oml = oml; bc.omeps = (float)(1.0 - eps); bc.q_off = (float)(eps / N);
    bc.thresh = thresh < 0.f ? -1.f : thresh; bc.k = k; bc.sum_classes = sum_classes != 0;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(sigmoid_bce_rows_kernel, dim3(B), dim3(256), (size_t)N * sizeof(float), st, z, ta, tb, gz, row_loss, row_hit,
                       row_hitk, B, N, bc);
    LOANS_LAUNCH_CHECK();
    hipLaunchKernelGGL(sigmoid_bce_reduce_kernel, dim3(1), dim3(256), 0, st, row_loss, row_hit, row_hitk, ta, tb, out, B, N,
                       bc.sum_classes);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_softmax_distill_fwd_f32(const float* z, const float* zt, const int32_t* ta, const int32_t* tb, float lam,
                                             float oml, float* gz, float* row_loss, float* row_hit, float* row_hitk,
                                             float* row_kl, float* row_thit, float* out, int32_t B, int32_t N, double eps,
                                             int32_t k, double alpha, double T, void* stream) {
    if (!z || !ta || !tb || !gz || !row_loss || !row_hit || !row_hitk || !row_kl || !row_thit || !out || B <= 0 || N <= 0)
        return LOANS_EINVAL;
    if (!(eps >= 0.0 && eps < 1.0) || k < 1 || !__builtin_isfinite(lam) || !__builtin_isfinite(oml)) return LOANS_EINVAL;
    if (!(alpha >= 0.0 && alpha <= 1.0) || !(T >= 0.015625 && T <= 64.0)) return LOANS_EINVAL;        // (a NaN too)
    if (alpha > 0.0 && !zt) return LOANS_EINVAL;
    if (N > XENT_MAX_N || B > XENT_MAX_B) return LOANS_ERANGE;
    hipStream_t st = as_stream(stream);
    if (alpha == 0.0) {         // the mix entry itself -- its bits -- and zeros; zt is not read
        if (int rc = loans_softmax_xent_mix_fwd_f32(z, ta, tb, lam, oml, gz, row_loss, row_hit, row_hitk, out, B, N, eps, k, stream))
            return rc;
        hipLaunchKernelGGL(softmax_distill_zero_kernel, dim3((B + 255) / 256), dim3(256), 0, st, row_kl, row_thit, out, B);
        LOANS_LAUNCH_CHECK();
        return LOANS_OK;
    }
    // one label per row: the array that carries the whole weight in both places, so the other one is not read
    if (lam == 1.f && oml == 0.f) tb = ta;
    if (lam == 0.f && oml == 1.f) ta = tb;
    Distill ds;
    ds.mx.ls.eps = (float)eps; ds.mx.ls.omeps = (float)(1.0 - eps); ds.mx.ls.q_off = (float)(eps / N);
    ds.mx.ls.q_on = ds.mx.ls.omeps + ds.mx.ls.q_off; ds.mx.ls.k = k; ds.mx.lam = lam; ds.mx.oml = oml;
    ds.invT = (float)(1.0 / T); ds.oma = (float)(1.0 - alpha); ds.alpha = (float)alpha; ds.T2 = (float)(T * T);
    ds.aT = (float)(alpha * T);
    hipLaunchKernelGGL(softmax_distill_rows_kernel, dim3(B), dim3(256), (size_t)N * sizeof(float), st, z, zt, ta, tb, gz, row_loss,
                       row_hit, row_hitk, row_kl, row_thit, B, N, ds);
    LOANS_LAUNCH_CHECK();
    hipLaunchKernelGGL(softmax_distill_reduce_kernel, dim3(1), dim3(256), 0, st, row_loss, row_hit, row_hitk, row_kl, row_thit, ta,
                       tb, out, B, N);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_softmax_xent_eval_f32(const float* z, const int32_t* t, float* rows, double* acc, int32_t B, int32_t N,
                                           int32_t k, void* stream) {
    if (!z || !t || !rows || !acc || B <= 0 || N <= 0 || k < 1) return LOANS_EINVAL;
    if (N > XENT_MAX_N || B > XENT_MAX_B) return LOANS_ERANGE;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(softmax_xent_eval_rows_kernel, dim3(B), dim3(256), (size_t)N * sizeof(float), st, z, t, rows, B, N, k);
    LOANS_LAUNCH_CHECK();
    hipLaunchKernelGGL(softmax_xent_eval_reduce_kernel, dim3(1), dim3(256), 0, st, rows, t, acc, B, N);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int loans_scale_by_scalar_f32(const float* x, const float* s, float* y, int64_t n, void* stream) {
    if (!x || !s || !y || n <= 0) return LOANS_EINVAL;
    hipLaunchKernelGGL(scale_by_scalar_kernel, dim3(grid_for(n, 256)), dim3(256), 0, as_stream(stream), x, s, y, n);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}
