// What the kernels over the flat parameter arena are made of (sgd.hip, lamb.hip, clip.hip; the four vector accesses misc.hip too),
// each piece once.  Every one of these kernels promises the same bits on every run: the order of the fp64 additions -- a thread's
// elements (float4 k ascending, lane e ascending), the xor butterfly 32, 16 .. 1 inside the wave, waves 0..3 through LDS, a
// segment's units ascending -- is written here and nowhere else.  Which buffer is non-temporal, and why, is said at each kernel.
#pragma once
#include "common.h"
#include "seg_table.h"

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ f32x4 ldnt4(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); }
__device__ __forceinline__ void stnt4(float* p, f32x4 v) { __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p)); }

constexpr int ARENA_UNIT = LOANS_LARS_UNIT;
typedef double f64x2 __attribute__((ext_vector_type(2)));       // a unit's two partial sums

// ---- units ------------------------------------------------------------------------------------------------------------------------
// Work is cut into units of ARENA_UNIT floats PER SEGMENT, one block per unit and trip (u, u + gridDim.x, ..): unit u belongs to the
// segment with the largest first_unit <= u (u is the same for the whole block: scalar loads), so a unit never straddles a boundary
// and a partial lands in ws[u] whichever block summed it.  A first_unit table that does not belong to these ends: touch nothing.
struct ArenaUnit { int seg; int64_t off, left; };      // floats [off, off + min(left, ARENA_UNIT)) of segment seg

__device__ __forceinline__ ArenaUnit arena_unit(const int64_t* __restrict__ seg_end, const int64_t* __restrict__ seg_first_unit,
                                                int nseg, int64_t u) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg_first_unit[mid] <= u) lo = mid; else hi = mid - 1;
    }
    const int64_t start = lo ? seg_end[lo - 1] : 0;
    const int64_t off = start + (u - seg_first_unit[lo]) * ARENA_UNIT;
    return {lo, off, off < start ? 0 : seg_end[lo] - off};
}

// One unit of p and of N streamed buffers, body(pe, x) once per element with pe that element of p and x[b] that of buf[b]; what
// body leaves in x[b] is stored where bit b of `wr` is set (a constant: the test folds away).  p is only read, and
// cacheable; the streamed buffers are read and written non-temporally (why, the kernels say).  A full unit is four float4 of every
// buffer per thread, ALL loads issued before the first use; a last, short unit takes float4 while they fit (stride 1024) and single
// floats for the n & 3 behind them (only the arena's end has those).  A thread visits k ascending, e ascending.  (grad_sumsq_kernel
// of clip.hip walks g alone and lamb_moments_kernel four buffers in the same order, written out; each says why.)
template <int N, class Body>
__device__ __forceinline__ void arena_walk(const float* __restrict__ p, float* const (&buf)[N], unsigned wr, int64_t off, int64_t left,
                                           Body body) {
    struct Quad { f32x4 p, x[N]; };
    auto load = [&](Quad& q, unsigned at) {             // `at` counts from the unit's first float: one uniform base per buffer
        q.p = ld4(p + off + at);
#pragma unroll
        for (int b = 0; b < N; ++b) q.x[b] = ldnt4(buf[b] + off + at);
    };
    auto visit = [&](Quad& q, unsigned at) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float y[N];
#pragma unroll
            for (int b = 0; b < N; ++b) y[b] = q.x[b][e];
            body(q.p[e], y);
#pragma unroll
            for (int b = 0; b < N; ++b) q.x[b][e] = y[b];
        }
#pragma unroll
        for (int b = 0; b < N; ++b)
            if (wr >> b & 1) stnt4(buf[b] + off + at, q.x[b]);
    };
    if (left >= ARENA_UNIT) {
        Quad q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) load(q[k], (k * 256 + threadIdx.x) * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) visit(q[k], (k * 256 + threadIdx.x) * 4);
    } else if (left > 0) {
        const int m = (int)left, m4 = m & ~3;
        for (int k = threadIdx.x * 4; k < m4; k += 1024) {
            Quad q;
            load(q, k);
            visit(q, k);
        }
        if ((int)threadIdx.x < (m & 3)) {
            const int64_t at = off + m4 + threadIdx.x;
            float y[N];
#pragma unroll
            for (int b = 0; b < N; ++b) y[b] = buf[b][at];
            body(p[at], y);
#pragma unroll
            for (int b = 0; b < N; ++b)
                if (wr >> b & 1) buf[b][at] = y[b];
        }
    }
}

// The block's NS fp64 sums (256 threads, sh: 4 * NS doubles): thread 0 stores them to dst as ONE vector, ((w0 + w1) + w2) + w3.
template <int NS>
__device__ __forceinline__ void arena_block_sums(double (&s)[NS], double* sh, double* dst) {
    typedef double Sums __attribute__((ext_vector_type(NS)));
#pragma unroll
    for (int j = 0; j < NS; ++j) s[j] = wave_sum_d(s[j]);
    __syncthreads();            // the previous trip's sh has been read
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < NS; ++j) sh[4 * j + (threadIdx.x >> 6)] = s[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Sums out;
#pragma unroll
        for (int j = 0; j < NS; ++j) out[j] = ((sh[4 * j] + sh[4 * j + 1]) + sh[4 * j + 2]) + sh[4 * j + 3];
        *reinterpret_cast<Sums*>(dst) = out;
    }
}

// ---- fold: the pair partials of segment blockIdx.x in ascending unit order, both sums in every lane ------------------------------
// One wave per segment (sh: 64 pairs).  The order of the additions is the units' -- one chain per sum --, but the loads are not on
// that chain: the wave fetches 64 partials at a time, one 16-byte load per lane, the next 64 before the current ones are added, and
// passes them through LDS to an unrolled loop.  (One thread per segment walking its partials alone waits for every load, 576 round
// trips for ResNet-50's largest tensor: LARS's two launches took 154 us that way, profiles/imagenet_lars.txt.)
__device__ __forceinline__ f64x2 arena_fold_segment(const f64x2* __restrict__ ws, const int64_t* __restrict__ seg_end,
                                                    const int64_t* __restrict__ seg_first_unit, int64_t units, f64x2* sh) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int64_t start = s ? seg_end[s - 1] : 0;
    const int64_t first = seg_first_unit[s];
    int64_t count = (seg_end[s] - start + ARENA_UNIT - 1) / ARENA_UNIT;
    if (first < 0 || first + count > units) count = 0;          // (a first_unit table that does not belong to these ends)
    const f64x2 zero = {0.0, 0.0};
    f64x2 sum = zero;
    f64x2 next = lane < count ? ws[first + lane] : zero;
    for (int64_t base = 0; base < count; base += 64) {
        sh[lane] = next;
        next = base + 64 + lane < count ? ws[first + base + 64 + lane] : zero;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 64; ++k) sum += sh[k];      // every lane carries the same chain (broadcast reads, no divergence); slots
        __syncthreads();                                // behind the last unit hold +0.0, which changes no bit of a non-negative sum
    }
    return sum;
}

// ---- segment cursor of the grid-stride updates --------------------------------------------------------------------------------
// The table -- exclusive ends, flags, and ratios where the kernel has them (ratio = seg_ratio = nullptr where not) -- is copied into
// LDS once per block, AFTER the first trip's loads have gone out: the grid is one wave of blocks, so a global load, a barrier and a
// bisection in front of every block's first load is time a plain kernel does not spend (1.3 us of 79 at the ResNet-50 arena,
// profiles/imagenet_ema.txt).  A thread bisects once for its first float4 and from there carries a cursor: the indices only grow, so
// the cursor only moves forward -- at most SEG_MAX_SEGMENTS LDS reads per thread over the whole launch, none on the path of the loads.
__device__ __forceinline__ void seg_load(int64_t* ends, uint8_t* flags, float* ratio, const int64_t* __restrict__ seg_end,
                                         const uint8_t* __restrict__ seg_flags, const float* __restrict__ seg_ratio, int nseg) {
    for (int s = threadIdx.x; s < nseg; s += 256) {
        ends[s] = seg_end[s]; flags[s] = seg_flags[s];
        if (ratio) ratio[s] = seg_ratio[s];
    }
}

// the first segment whose end lies behind float `at`
__device__ __forceinline__ int seg_find(const int64_t* ends, int nseg, int64_t at) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ends[mid] > at) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ int seg_advance(const int64_t* ends, int nseg, int seg, int64_t at) {
    while (seg < nseg - 1 && ends[seg] <= at) ++seg;            // (the last end is n > at)
    return seg;
}
