// Element types of the data matrix X.  Every kernel that reads X has ONE body, a template over a load policy:
//   XF32   the fp32 kernels (a float4 load, used as loaded)
//   XBF16  bf16 storage:  the same 4 elements as one 8-byte load; to fp32 by a 16-bit shift
//   XF16   fp16 storage:  the same 4 elements as one 8-byte load; to fp32 by v_cvt_f32_f16
// Both conversions are exact, so everything after the load - LDS image, MFMA fragments, order of accumulation - sees the
// values the fp32 kernel sees for X.float(): a run on 16-bit X gives bit for bit the fp32 run on the upcast matrix.
// Prefetching kernels keep the RAW registers in flight (half the VGPRs of a float4) and convert where the fp32 kernel
// consumes its float4, so no conversion waits on a load earlier than the fp32 kernel's use would.
#pragma once
#include <cstdint>
#include <type_traits>

#include "mcl_internal.h"

typedef float mcl_xf32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int mcl_xu32x2 __attribute__((ext_vector_type(2)));

struct XF32 {
    using T = float;
    using raw = mcl_xf32x4;
    static constexpr const char *name = "f32";
    template <bool NT>
    static __device__ __forceinline__ raw ld4(const float *p) {
        return NT ? __builtin_nontemporal_load(reinterpret_cast<const raw *>(p)) : *reinterpret_cast<const raw *>(p);
    }
    static __device__ __forceinline__ mcl_xf32x4 cvt(raw v) { return v; }
    static __device__ __forceinline__ float ld1(const float *p) { return *p; }
};

struct XBF16 {
    using T = uint16_t;
    using raw = mcl_xu32x2;
    static constexpr const char *name = "bf16";
    template <bool NT>
    static __device__ __forceinline__ raw ld4(const uint16_t *p) {
        return NT ? __builtin_nontemporal_load(reinterpret_cast<const raw *>(p)) : *reinterpret_cast<const raw *>(p);
    }
    static __device__ __forceinline__ mcl_xf32x4 cvt(raw v) {
        return mcl_xf32x4{__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16),
                          __uint_as_float(v.y & 0xffff0000u)};
    }
    static __device__ __forceinline__ float ld1(const uint16_t *p) { return __uint_as_float((unsigned)*p << 16); }
};

struct XF16 {
    using T = uint16_t;
    using raw = mcl_xu32x2;
    static constexpr const char *name = "f16";
    template <bool NT>
    static __device__ __forceinline__ raw ld4(const uint16_t *p) {
        return NT ? __builtin_nontemporal_load(reinterpret_cast<const raw *>(p)) : *reinterpret_cast<const raw *>(p);
    }
    static __device__ __forceinline__ float h(unsigned bits) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits); }
    static __device__ __forceinline__ mcl_xf32x4 cvt(raw v) { return mcl_xf32x4{h(v.x), h(v.x >> 16), h(v.y), h(v.y >> 16)}; }
    static __device__ __forceinline__ float ld1(const uint16_t *p) { return h(*p); }
};

// fp64 data a kernel keeps for itself (the filled copy X~ of csrc/multistart.hip's missing-entry fit): element loads only, no
// vector form and no place in mcl_x_dispatch - no caller stores X in fp64
struct XF64 {
    using T = double;
    static constexpr const char *name = "f64";
    static __device__ __forceinline__ double ld1(const double *p) { return *p; }
};

// register image of four elements: the raw vector load, or (V = false: the non-vectorised paths, element by element
// through ld1) four fp32 values
template <class XL, bool V>
using xraw_t = std::conditional_t<V, typename XL::raw, mcl_xf32x4>;
template <class XL, bool V>
static __device__ __forceinline__ mcl_xf32x4 xcvt(xraw_t<XL, V> v) {
    if constexpr (V) return XL::cvt(v);
    else return v;
}

// launch-site dispatch on the context's element type: f(XF32{}) / f(XBF16{}) / f(XF16{})
template <class F>
static inline auto mcl_x_dispatch(int x_type, F &&f) {
    if (x_type == MCL_X_BF16) return f(XBF16{});
    if (x_type == MCL_X_F16) return f(XF16{});
    return f(XF32{});
}
// the kernel NAME<ARGS> of the launch site's element type XL: NAME<ARGS> for fp32, its twin NAME_h<XL, ARGS> for 16 bits
// (only the selected one is instantiated)
#define MCL_XKERNEL(NAME, ...)                                             \
    ([]() {                                                                \
        if constexpr (std::is_same_v<XL, XF32>) return NAME<__VA_ARGS__>; \
        else return NAME##_h<XL, __VA_ARGS__>;                             \
    }())
// the same for a kernel that is no template in its fp32 form: NAME, or NAME_h<XL>
#define MCL_XKERNEL0(NAME)                                    \
    ([]() {                                                   \
        if constexpr (std::is_same_v<XL, XF32>) return NAME; \
        else return NAME##_h<XL>;                             \
    }())
template <class XL>
static inline const typename XL::T *mcl_x(const mcl_context *c) { return static_cast<const typename XL::T *>(c->X); }
// X's base allows the vector loads: 16 bytes for a float4, 8 for four 16-bit elements
static inline bool mcl_x_vec_aligned(const void *X, int x_type) {
    return (reinterpret_cast<uintptr_t>(X) & (x_type == MCL_X_F32 ? 15 : 7)) == 0;
}
static inline bool mcl_x_vec_aligned(const mcl_context *c) { return mcl_x_vec_aligned(c->X, c->x_type); }
// kernel_variant strings: "k_name<ARGS>" for fp32, "k_name_h<bf16,ARGS>" / "k_name_h<f16,ARGS>" for the twins
template <class XL>
static inline const char *mcl_x_kname() { return std::is_same_v<XL, XF32> ? "" : "_h"; }
template <class XL>
static inline const char *mcl_x_targ() { return std::is_same_v<XL, XBF16> ? "bf16," : std::is_same_v<XL, XF16> ? "f16," : ""; }
