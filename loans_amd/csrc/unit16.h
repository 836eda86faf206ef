// The 16-byte unit of the streaming BN / junction passes (bn_pool.hip, se.hip): 4 fp32 or 8 bf16 channels of an NHWC tensor as
// fp32 vectors, and the sign-bit bytes that go with them.  Not part of the C ABI.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 relu4(f32x4 v) {
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    return v;
}

// signbits (optional): one byte per four channels, bit e = (y[4i + e] > 0) -- the ReLU mask the backward passes of this BN
// need, at 1/16 (fp32) or 1/8 (bf16) of the bytes of y
__device__ __forceinline__ uint8_t posbits4(f32x4 v) {
    return (uint8_t)((v.x > 0.f ? 1 : 0) | (v.y > 0.f ? 2 : 0) | (v.z > 0.f ? 4 : 0) | (v.w > 0.f ? 8 : 0));
}
__device__ __forceinline__ f32x4 maskbits4(f32x4 g, uint8_t m) {
    g.x = (m & 1) ? g.x : 0.f; g.y = (m & 2) ? g.y : 0.f;
    g.z = (m & 4) ? g.z : 0.f; g.w = (m & 8) ? g.w : 0.f;
    return g;
}

template <typename T> struct unit16;
template <> struct unit16<float> {
    static constexpr int V = 4, NV = 1;
    typedef f32x4 raw_t;
    template <bool NT = false> static __device__ __forceinline__ raw_t ldr(const float* p) {
        if (NT) return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
        return *reinterpret_cast<const f32x4*>(p);
    }
    static __device__ __forceinline__ void cvt(raw_t r, f32x4* v) { v[0] = r; }
    static __device__ __forceinline__ void ld(const float* p, f32x4* v) { v[0] = *reinterpret_cast<const f32x4*>(p); }
    template <bool NT = false> static __device__ __forceinline__ void st(float* p, const f32x4* v) {
        if (NT) __builtin_nontemporal_store(v[0], reinterpret_cast<f32x4*>(p));
        else *reinterpret_cast<f32x4*>(p) = v[0];
    }
};
template <> struct unit16<__bf16> {
    static constexpr int V = 8, NV = 2;
    typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
    typedef bf16x8 raw_t;
    template <bool NT = false> static __device__ __forceinline__ raw_t ldr(const __bf16* p) {
        if (NT) return __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(p));
        return *reinterpret_cast<const bf16x8*>(p);
    }
    static __device__ __forceinline__ void cvt(raw_t r, f32x4* v) {
        v[0] = __builtin_convertvector(__builtin_shufflevector(r, r, 0, 1, 2, 3), f32x4);
        v[1] = __builtin_convertvector(__builtin_shufflevector(r, r, 4, 5, 6, 7), f32x4);
    }
    static __device__ __forceinline__ void ld(const __bf16* p, f32x4* v) { cvt(ldr(p), v); }
    template <bool NT = false> static __device__ __forceinline__ void st(__bf16* p, const f32x4* v) {
        const loans_bf16x4 a = __builtin_convertvector(v[0], loans_bf16x4), b = __builtin_convertvector(v[1], loans_bf16x4);
        const bf16x8 r = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
        if (NT) __builtin_nontemporal_store(r, reinterpret_cast<bf16x8*>(p));
        else *reinterpret_cast<bf16x8*>(p) = r;
    }
};


// one byte of sign bits per four channels: a unit owns NV consecutive bytes
template <int NV> __device__ __forceinline__ void st_bits(uint8_t* p, const f32x4* v) {
    if (NV == 1) p[0] = posbits4(v[0]);
    else *reinterpret_cast<uint16_t*>(p) = (uint16_t)(posbits4(v[0]) | (posbits4(v[1]) << 8));
}
template <int NV> __device__ __forceinline__ void ld_bits(const uint8_t* p, uint8_t* b) {
    if (NV == 1) b[0] = p[0];
    else { const uint16_t w = *reinterpret_cast<const uint16_t*>(p); b[0] = (uint8_t)(w & 255); b[1] = (uint8_t)(w >> 8); }
}

constexpr int SLAB_UNR = 4;     // units a thread keeps in flight (bn_pool.hip: "The units one block streams")
// LOANS_BN_NT: 0 never, 1 always, unset: tensors of at least 96 MB (they cannot stay in the Infinity Cache with their partners)
static inline bool slab_nt(int64_t tensor_bytes) {
    static const int mode = [] { const char* e = getenv("LOANS_BN_NT"); return e && *e ? atoi(e) : -1; }();
    constexpr long mb = 96;
    return mode < 0 ? tensor_bytes >= ((int64_t)mb << 20) : mode != 0;
}

}  // namespace
