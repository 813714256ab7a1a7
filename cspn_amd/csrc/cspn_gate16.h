// cspn_gate16.h -- the gate storage type GT of the engines that take fp16 / bf16 gates (cspn2d_kxk.hip, the 3D kernels): float, or __half /
// __hip_bfloat16 (the *_g16 entry points).  A 16-bit gate is widened to float32 exactly where it is read (fp16 subnormals kept, bf16 = its
// bits shifted left by 16), so every result is bitwise the float32 kernel's on the widened gates; a gradient with respect to a 16-bit tensor
// is accumulated in float32 and rounded once, to nearest even, at its single store.
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <type_traits>

#include "../../include/cspn_amd.h"

namespace cspn {

// ---- the gate storage type.  A 16-bit gate travels as its bit pattern (unsigned short); float gates as themselves ----
template <class GT>
struct Store {
    using type = unsigned short;
};
template <>
struct Store<float> {
    using type = float;
};
template <class GT>
using store_t = typename Store<GT>::type;

// exact widening of a stored gate
template <class GT>
__device__ __forceinline__ float widen(store_t<GT> v) {
    if constexpr (std::is_same<GT, float>::value) return v;
    else if constexpr (std::is_same<GT, __half>::value) return (float)__builtin_bit_cast(_Float16, v);
    else return __uint_as_float((uint32_t)v << 16);
}

// the single rounding of a float32 gradient to the storage type: to nearest even, subnormals kept, NaN stays NaN
template <class GT>
__device__ __forceinline__ store_t<GT> narrow(float v) {
    if constexpr (std::is_same<GT, float>::value) return v;
    else if constexpr (std::is_same<GT, __half>::value) return __builtin_bit_cast(unsigned short, (_Float16)v);
    else {
        const uint32_t u = __float_as_uint(v);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)0x7fc0;
        return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
}

// four consecutive gates as float32: one 16-byte (float) or 8-byte (16-bit) access at that alignment; ld4gu: aligned to one element only
template <class GT>
__device__ __forceinline__ float4 widen4(uint2 q) {
    return make_float4(widen<GT>((unsigned short)q.x), widen<GT>((unsigned short)(q.x >> 16)), widen<GT>((unsigned short)q.y),
                       widen<GT>((unsigned short)(q.y >> 16)));
}

template <class GT>
__device__ __forceinline__ float4 ld4g(const store_t<GT>* p) {
    if constexpr (std::is_same<GT, float>::value) return *reinterpret_cast<const float4*>(p);
    else return widen4<GT>(*reinterpret_cast<const uint2*>(p));
}

template <class GT>
__device__ __forceinline__ float4 ld4gu(const store_t<GT>* p) {
    if constexpr (std::is_same<GT, float>::value) {
        float4 v;
        __builtin_memcpy(&v, p, 16);
        return v;
    } else {
        uint2 q;
        __builtin_memcpy(&q, p, 8);
        return widen4<GT>(q);
    }
}

template <class GT>
__device__ __forceinline__ void st4g(store_t<GT>* p, float a, float b, float c, float d) {
    if constexpr (std::is_same<GT, float>::value) *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
    else
        *reinterpret_cast<uint2*>(p) = make_uint2((uint32_t)narrow<GT>(a) | ((uint32_t)narrow<GT>(b) << 16),
                                                  (uint32_t)narrow<GT>(c) | ((uint32_t)narrow<GT>(d) << 16));
}

// host side: f(Tag<GT>{}) for the storage type of `dtype` (0 float32, CSPN_DTYPE_F16, CSPN_DTYPE_BF16: checked by the caller)
template <class GT>
struct Tag {
    using type = GT;
};

template <class F>
auto with_gate_type(int dtype, F f) {
    if (dtype == 0) return f(Tag<float>{});
    if (dtype == CSPN_DTYPE_F16) return f(Tag<__half>{});
    return f(Tag<__hip_bfloat16>{});
}

// bytes of a stored gate, and the alignment mask of four of them (the vector paths' condition on a gate pointer)
inline size_t gate_bytes(int dtype) { return dtype == 0 ? 4 : 2; }
inline uintptr_t gate_quad_mask(int dtype) { return dtype == 0 ? 15u : 7u; }

// the vector kernels' condition: four voxels of a thread share a row, every float32 tensor of the call is 16-byte aligned and the
// gate-typed ones to four of their elements (16 bytes, or 8 for a 16-bit type); NULL: absent.  Each caller lists its own tensors
inline bool quads_ok(int W, int gdt, std::initializer_list<const void*> gates, std::initializer_list<const void*> tensors) {
    uintptr_t gbits = 0, bits = 0;
    for (const void* t : gates) gbits |= (uintptr_t)t;
    for (const void* t : tensors) bits |= (uintptr_t)t;
    return (W % 4) == 0 && (gbits & gate_quad_mask(gdt)) == 0 && (bits & 15u) == 0;
}

}  // namespace cspn
