// The wide Linear layer (the ImageNet / ImageNet-21k classification head) on the bf16 matrix cores: forward, data gradient and
// weight gradient of loans_linear_wide16_*_f32.  Every tensor is fp32 in memory; an operand element is rounded to bf16 (nearest
// even) on its way into LDS, products and sums are fp32 in the accumulators of v_mfma_f32_32x32x16_bf16.
//
// ONE kernel, head16_kernel, for  out(m, c) (+)= sum_r A(m, r) Bm(r, c)  with either operand reduction-contiguous or not:
//   forward          y[b][n]  = sum_k x[b][k] W[n][k] + bias     m = b, c = n, r = k    A and Bm reduction-contiguous
//   data gradient    gx[b][k] = sum_n gy[b][n] W[n][k]           m = b, c = k, r = n    A reduction-contiguous, Bm column-contiguous;
//                    the class axis is cut into slices, slice s stores its tile into slab s, head16_fold_kernel sums the slabs
//   weight gradient  gW[n][k] += sum_b x[b][k] gy[b][n]          m = k, c = n, r = b    both row / column-contiguous; the tile is
//                    computed TRANSPOSED (rows = k), so that the four accumulator registers an MFMA lane holds for consecutive
//                    rows are four consecutive k of one class: gW is read and written once, 16 bytes per access
// Block = 4 waves = a 128 x 128 tile (2 x 2 waves of 2 x 2 MFMA tiles), the reduction in chunks of 32 through two LDS stages:
//   * a thread fetches 4 consecutive floats (16 bytes where the row pitch and the base allow it, four dwords otherwise -- gy has
//     rows of N floats, any N), 4 such per operand and chunk, converts them in registers and stores 8 bytes of bf16;
//   * a reduction-contiguous operand lies in LDS as [element][32 r] with a pitch of 40 bf16 (80 bytes: the sixteen 16-byte
//     fragment reads of a quarter wave start 20 banks apart and cover all 64 banks once), a lane reads its 8 consecutive r with
//     one ds_read_b128;
//   * the other kind lies as it does in memory, [32 r][128 elements] with a pitch of 160 bf16, and is read with the hardware
//     transpose ds_read_b64_tr_b16 exactly as the weight gradient of igemm_bf16.hip does (two reads are one fragment);
//   * the loads of chunk i + 1 are issued before the MFMAs of chunk i and stored to the other stage after them: one barrier per
//     chunk.
// Rows, columns and reduction indices past an edge (or past the end of a slice) are staged as zeros, so a ragged tile sums
// exactly its own terms.  No atomics: every output element is owned by one lane and summed in an order fixed by the shape.
#include "common.h"

namespace {

typedef __bf16 h_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 h_bf16x4 __attribute__((ext_vector_type(4)));

constexpr int HT = 128;             // tile edge (rows and columns of `out`)
constexpr int HK = 32;              // reduction chunk
constexpr int HP_RC = HK + 8;       // LDS pitch of a reduction-contiguous operand, [HT][HP_RC] bf16
constexpr int HP_T = HT + 32;       // LDS pitch of the other kind, [HK][HP_T] bf16
constexpr int HSTAGE = HT * HP_RC;  // bf16 per operand and stage
static_assert(HK * HP_T == HSTAGE, "both LDS images of an operand have one size");
constexpr int HLOADS = HT * HK / 4 / 256;       // 16-byte loads per thread, operand and chunk

constexpr int SPLIT_BLOCKS = 256;   // the data gradient aims at this many blocks ...
constexpr int SPLIT_MIN_CHUNKS = 4; // ... of at least this many chunks each

enum { EPI_FWD = 0, EPI_SLAB = 1, EPI_WGRAD = 2 };

struct Head16Args {
    const float* A;     // A_RC: A[m * lda + r], else A[r * lda + m]
    const float* Bm;    // B_RC: Bm[c * ldb + r], else Bm[r * ldb + c]
    const float* bias;  // EPI_FWD: [C] or NULL
    float* out;         // EPI_FWD: out[m * ldo + c];  EPI_SLAB: slab s at out + s * M * C, [m][c];  EPI_WGRAD: out[c * ldo + m]
    int lda, ldb, ldo;
    int M, C, R;
    int chunks_per_slice;   // slice blockIdx.z reduces over chunks [z * chunks_per_slice, ...) of the R axis
    int vecA, vecB, vecO;   // 16-byte accesses are legal on that tensor (base and row pitch multiples of 16 bytes)
};

// four consecutive floats p[0 .. 3], the first n of them inside the tensor (n <= 0: none), the others zero
__device__ __forceinline__ f32x4 load4(const float* __restrict__ p, int n, int vec) {
    if (n >= 4 && vec) return *reinterpret_cast<const f32x4*>(p);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (n > 0) v.x = p[0];
    if (n > 1) v.y = p[1];
    if (n > 2) v.z = p[2];
    if (n > 3) v.w = p[3];
    return v;
}

// one operand's share of a chunk in registers: element range [e0, e0 + HT) of E, reduction range [r0, r0 + HK) below r_end
template <bool RC>
__device__ __forceinline__ void fetch(const float* __restrict__ src, int ld, int e0, int E, int r0, int r_end, int vec,
                                      f32x4 (&v)[HLOADS], int tid) {
#pragma unroll
    for (int i = 0; i < HLOADS; ++i) {
        if (RC) {       // 8 threads walk the 32 r of one element
            const int ge = e0 + (tid >> 3) + 32 * i, gr = r0 + (tid & 7) * 4;
            v[i] = load4(src + (int64_t)ge * ld + gr, ge < E ? r_end - gr : 0, vec);
        } else {        // 32 threads walk the 128 elements of one r
            const int ge = e0 + (tid & 31) * 4, gr = r0 + (tid >> 5) + 8 * i;
            v[i] = load4(src + (int64_t)gr * ld + ge, gr < r_end ? E - ge : 0, vec);
        }
    }
}

template <bool RC>
__device__ __forceinline__ void stash(__bf16* dst, const f32x4 (&v)[HLOADS], int tid) {
#pragma unroll
    for (int i = 0; i < HLOADS; ++i) {
        const int at = RC ? ((tid >> 3) + 32 * i) * HP_RC + (tid & 7) * 4 : ((tid >> 5) + 8 * i) * HP_T + (tid & 31) * 4;
        *reinterpret_cast<h_bf16x4*>(dst + at) = __builtin_convertvector(v[i], h_bf16x4);       // round to nearest even
    }
}

// the fragment of MFMA tile `t` (32 elements from `base`) for reduction step s (16 r) of the staged chunk
template <bool RC>
__device__ __forceinline__ h_bf16x8 fragment(const __bf16* st, int base, int s, int lane) {
    if (RC) return *reinterpret_cast<const h_bf16x8*>(st + (base + (lane & 31)) * HP_RC + 16 * s + 8 * (lane >> 5));
    // 16-lane group g: reduction rows 8 * (g >> 1) + 0 .. 3 (and + 4 .. 7), elements 16 * (g & 1) .. + 15; lane 4q + p of the group
    // addresses row q, elements 4p .. 4p + 3 and receives element (lane & 15) of the four rows
    typedef __attribute__((address_space(3))) h_bf16x4* lds_b64_t;
    const int li = lane & 15, g = lane >> 4;
    const __bf16* p = st + (16 * s + 8 * (g >> 1) + (li >> 2)) * HP_T + base + 16 * (g & 1) + 4 * (li & 3);
    const h_bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b64_t)p);
    const h_bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b64_t)(p + 4 * HP_T));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// grid: x = row tiles (adjacent in launch order: at M <= 256 the two blocks that share a column range of Bm run together and the
// second finds it in L2), y = column tiles, z = slices of the reduction
template <bool A_RC, bool B_RC, int EPI>
__global__ __launch_bounds__(256) void head16_kernel(const Head16Args a) {
    __shared__ __attribute__((aligned(16))) __bf16 As[2][HSTAGE];
    __shared__ __attribute__((aligned(16))) __bf16 Bs[2][HSTAGE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * HT, c0 = blockIdx.y * HT;
    const int chunks = (a.R + HK - 1) / HK;
    const int ch_begin = blockIdx.z * a.chunks_per_slice;
    const int ch_end = min(ch_begin + a.chunks_per_slice, chunks);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    f32x4 va[HLOADS], vb[HLOADS];
    if (ch_begin < ch_end) {
        fetch<A_RC>(a.A, a.lda, m0, a.M, ch_begin * HK, a.R, a.vecA, va, tid);
        fetch<B_RC>(a.Bm, a.ldb, c0, a.C, ch_begin * HK, a.R, a.vecB, vb, tid);
        stash<A_RC>(As[0], va, tid);
        stash<B_RC>(Bs[0], vb, tid);
    }
    __syncthreads();
    for (int ch = ch_begin; ch < ch_end; ++ch) {
        const int buf = (ch - ch_begin) & 1;
        const bool more = ch + 1 < ch_end;
        if (more) {
            fetch<A_RC>(a.A, a.lda, m0, a.M, (ch + 1) * HK, a.R, a.vecA, va, tid);
            fetch<B_RC>(a.Bm, a.ldb, c0, a.C, (ch + 1) * HK, a.R, a.vecB, vb, tid);
        }
#pragma unroll
        for (int s = 0; s < HK / 16; ++s) {
            h_bf16x8 af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = fragment<A_RC>(As[buf], wm * 64 + i * 32, s, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = fragment<B_RC>(Bs[buf], wn * 64 + j * 32, s, lane);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        if (more) {
            stash<A_RC>(As[buf ^ 1], va, tid);
            stash<B_RC>(Bs[buf ^ 1], vb, tid);
        }
        __syncthreads();
    }

    // accumulator register e of lane (r, h): row (e & 3) + 8 * (e >> 2) + 4 * h, column r of the 32 x 32 tile
    float* const out = EPI == EPI_SLAB ? a.out + (int64_t)blockIdx.z * a.M * a.C : a.out;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = c0 + wn * 64 + j * 32 + r;
            if (c >= a.C) continue;
            if (EPI == EPI_WGRAD) {     // four consecutive rows are four consecutive floats of out[c][.]; M % 4 == 0
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int m = m0 + wm * 64 + i * 32 + 8 * q + 4 * h;
                    if (m >= a.M) continue;
                    float* o = out + (int64_t)c * a.ldo + m;
                    const f32x4 t = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                    if (a.vecO) {
                        *reinterpret_cast<f32x4*>(o) = *reinterpret_cast<const f32x4*>(o) + t;
                    } else {
                        o[0] += t.x; o[1] += t.y; o[2] += t.z; o[3] += t.w;
                    }
                }
            } else {
                const float bv = (EPI == EPI_FWD && a.bias) ? a.bias[c] : 0.f;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int m = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (m < a.M) out[(int64_t)m * a.ldo + c] = acc[i][j][e] + bv;
                }
            }
        }
}

// gx[i] = slab 0 [i] + slab 1 [i] + ... in slice order; n4 groups of four floats
__global__ __launch_bounds__(256) void head16_fold_kernel(const float* __restrict__ ws, float* __restrict__ gx, int64_t n4, int slices, int vec) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 s = *reinterpret_cast<const f32x4*>(ws + 4 * i);
        for (int k = 1; k < slices; ++k) s += *reinterpret_cast<const f32x4*>(ws + (k * n4 + i) * 4);
        if (vec) {
            *reinterpret_cast<f32x4*>(gx + 4 * i) = s;
        } else {
            gx[4 * i] = s.x; gx[4 * i + 1] = s.y; gx[4 * i + 2] = s.z; gx[4 * i + 3] = s.w;
        }
    }
}

int ceil_div(int a, int b) { return (a + b - 1) / b; }

// the data gradient's split of the class axis (include/loans_hip.h states the rule): -> chunks per slice, *slices
int plan_split(int B, int K, int N, int* slices) {
    const int chunks = ceil_div(N, HK), tiles = ceil_div(B, HT) * ceil_div(K, HT);
    int want = ceil_div(SPLIT_BLOCKS, tiles);
    if (want > ceil_div(chunks, SPLIT_MIN_CHUNKS)) want = ceil_div(chunks, SPLIT_MIN_CHUNKS);
    if (want < 1) want = 1;
    const int per = ceil_div(chunks, want);
    *slices = ceil_div(chunks, per);
    return per;
}

int vec_ok(const void* p, int ld) { return ((uintptr_t)p & 15) == 0 && (ld & 3) == 0; }

}  // namespace

extern "C" int loans_linear_wide16_fwd_f32(const float* x, const float* W, const float* b, float* y, int32_t B, int32_t K,
                                           int32_t N, void* stream) {
    if (!x || !W || !y) return LOANS_EINVAL;
    if (int rc = loans_wide_shape_ok(B, K, N)) return rc;
    Head16Args a = {x, W, b, y, K, K, N, B, N, K, ceil_div(K, HK), vec_ok(x, K), vec_ok(W, K), 0};
    hipLaunchKernelGGL((head16_kernel<true, true, EPI_FWD>), dim3(ceil_div(B, HT), ceil_div(N, HT), 1), dim3(256), 0, as_stream(stream), a);
    LOANS_LAUNCH_CHECK();
    return LOANS_OK;
}

extern "C" int64_t loans_linear_wide16_workspace(int32_t B, int32_t K, int32_t N) {
    if (int rc = loans_wide_shape_ok(B, K, N)) return rc;
    int slices = 1;
    plan_split(B, K, N, &slices);
    return slices > 1 ? (int64_t)slices * B * K * (int64_t)sizeof(float) : 0;
}

extern "C" int loans_linear_wide16_bwd_f32(const float* x, const float* W, const float* gy, float* gx, float* gW, float* gb,
                                           void* workspace, int64_t workspace_bytes, int32_t B, int32_t K, int32_t N, void* stream) {
    if (!gy) return LOANS_EINVAL;
    if ((gx && !W) || (gW && !x)) return LOANS_EINVAL;
    if (!gx && !gW && !gb) return LOANS_EINVAL;
    if (int rc = loans_wide_shape_ok(B, K, N)) return rc;
    int slices = 1;
    const int per = plan_split(B, K, N, &slices);
    if (gx && slices > 1) {
        if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < (int64_t)slices * B * K * (int64_t)sizeof(float)) return LOANS_EINVAL;
    }
    hipStream_t st = as_stream(stream);
    if (gx) {       // gx[b][k] = sum_n gy[b][n] W[n][k]: slabs per class slice, folded in slice order
        float* dst = slices > 1 ? (float*)workspace : gx;
        Head16Args a = {gy, W, nullptr, dst, N, K, K, B, K, N, per, vec_ok(gy, N), vec_ok(W, K), 0};
        hipLaunchKernelGGL((head16_kernel<true, false, EPI_SLAB>), dim3(ceil_div(B, HT), ceil_div(K, HT), slices), dim3(256), 0, st, a);
        LOANS_LAUNCH_CHECK();
        if (slices > 1) {
            const int64_t n4 = (int64_t)B * K / 4;
            hipLaunchKernelGGL(head16_fold_kernel, dim3(grid_for(n4, 256)), dim3(256), 0, st, (const float*)workspace, gx, n4, slices,
                               vec_ok(gx, 4));
            LOANS_LAUNCH_CHECK();
        }
    }
    if (gW) {       // gW[n][k] += sum_b x[b][k] gy[b][n], the tile transposed: rows = k
        Head16Args a = {x, gy, nullptr, gW, K, N, K, K, N, B, ceil_div(B, HK), vec_ok(x, K), vec_ok(gy, N), vec_ok(gW, K)};
        hipLaunchKernelGGL((head16_kernel<false, false, EPI_WGRAD>), dim3(ceil_div(K, HT), ceil_div(N, HT), 1), dim3(256), 0, st, a);
        LOANS_LAUNCH_CHECK();
    }
    if (gb) {       // from the unrounded gy: the fp32 entry's kernel and bits
        if (int rc = loans_colsum_ordered_launch(gy, gb, B, N, st)) return rc;
    }
    return LOANS_OK;
}
