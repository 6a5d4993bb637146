// The rule of the mix launch (mj_mix; tools/mix_model.py), shared by k_mix (mix.hip) and its host twin mj_host_mix: the element
// conversions, MixUp's three float32 operations, and which elements of a slot a CutMix box covers in each layout.
//
// MixUp, per element, with ws = float32(lam) and wp = float32(1.0 - lam) (the subtraction in double, then one rounding):
//     out = T( f32(T(f32(partner) * wp)) + f32(T(f32(self) * ws)) )
// T: round to nearest even into the output's element type; every float32 operation rounded on its own — the file is built with
// -ffp-contract=off and the products are never fused into the sum.  That is torch's x.roll(1, 0).mul(1.0 - lam).add_(x.mul(lam))
// on the CPU, bit for bit, in float32, float16 and bfloat16; a NaN result is some NaN.
//
// CutMix: a slot is one ow x oh canvas of C components in one of the four layouts (erase_addr.h's EraseCanvas), made of LINES of
// `len` contiguous elements — rows of ow pixels in the row-major layouts, columns of oh pixels in the x-major ones; `group`
// elements per pixel (C interleaved, 1 planar); `lines` of them per plane, the planar layouts' C planes one behind the other.
// Element e of the slot lies in line (e / len) % lines at offset e % len, and the box covers lines l0 .. l0 + ln - 1 at offsets
// o0 .. o0 + on - 1: two unsigned comparisons per element, and no division where line and offset are carried along.
#pragma once
#include <stdint.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "erase_addr.h"

namespace mj {

constexpr int kMixNone = 0, kMixMixup = 1, kMixCutmix = 2;      // MJ_MIX_*
constexpr int kDtypeU8 = 0, kDtypeF16 = 1, kDtypeBF16 = 2, kDtypeF32 = 3;      // MJ_DTYPE_*

// mj_mix_op checked and resolved: what the launch and the host twin take per output
struct DevMixOp {
    int32_t kind, partner;
    int32_t x, y, w, h;         // CUTMIX
    float ws, wp;               // MIXUP: the output's own weight and its partner's
};

__host__ __device__ inline float mix_bits_f32(uint32_t u) {
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(u);
#else
    float f; memcpy(&f, &u, 4); return f;
#endif
}
__host__ __device__ inline uint32_t mix_f32_bits(float f) {
#ifdef __HIP_DEVICE_COMPILE__
    return __float_as_uint(f);
#else
    uint32_t u; memcpy(&u, &f, 4); return u;
#endif
}

// float16 bits -> float32 (exact)
__host__ __device__ inline float mix_half_f32(uint32_t h) {
#ifdef __HIP_DEVICE_COMPILE__
    return (float)__builtin_bit_cast(_Float16, (uint16_t)h);
#else
    const uint32_t sign = (h & 0x8000u) << 16, em = h & 0x7FFFu;
    if (em >= 0x7C00u) return mix_bits_f32(sign | 0x7F800000u | ((em & 0x3FFu) << 13));       // infinity, NaN
    if (em >= 0x0400u) return mix_bits_f32(sign | ((em << 13) + 0x38000000u));
    const float m = (float)em * 5.9604644775390625e-8f;                                         // subnormal: em * 2^-24, exact
    return mix_bits_f32(sign | mix_f32_bits(m));
#endif
}
// float32 -> float16 bits, round to nearest even (overflow to infinity, gradual underflow)
__host__ __device__ inline uint32_t mix_f32_half(float f) {
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f);
#else
    const uint32_t x = mix_f32_bits(f), sign = (x >> 16) & 0x8000u, m = x & 0x7FFFFFFFu;
    if (m > 0x7F800000u) return sign | 0x7E00u;
    if (m >= 0x477FF000u) return sign | 0x7C00u;
    if (m < 0x38800000u) {
        // below 2^-14: adding 0.5 leaves the value in units of 2^-24 in the low mantissa bits, rounded by the addition itself
        volatile float sum = mix_bits_f32(m) + 0.5f;
        return sign | (mix_f32_bits(sum) - 0x3F000000u);
    }
    return sign | ((m - 0x38000000u + 0xFFFu + ((m >> 13) & 1u)) >> 13);
#endif
}
__host__ __device__ inline uint32_t mix_f32_bfloat(float f) {
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)f);       // (v_cvt_pk_bf16_f32: nearest even, a NaN stays a NaN)
#else
    const uint32_t x = mix_f32_bits(f);
    if ((x & 0x7FFFFFFFu) > 0x7F800000u) return (x >> 16) | 0x40u;
    return (x + 0x7FFFu + ((x >> 16) & 1u)) >> 16;
#endif
}

// an element's bits (in the low bytes) as float32, and float32 rounded into the element type, for the float MJ_DTYPE_* DT
template <int DT> __host__ __device__ inline float mix_load(uint32_t bits) {
    if constexpr (DT == kDtypeF32) return mix_bits_f32(bits);
    else if constexpr (DT == kDtypeF16) return mix_half_f32(bits);
    else return mix_bits_f32(bits << 16);
}
template <int DT> __host__ __device__ inline uint32_t mix_store(float f) {
    if constexpr (DT == kDtypeF32) return mix_f32_bits(f);
    else if constexpr (DT == kDtypeF16) return mix_f32_half(f);
    else return mix_f32_bfloat(f);
}

// the three operations: two products, each rounded to float32 and then to the element type, and their sum, rounded likewise
// (On the device every float32 result is pinned to a register before it is converted: left alone, the compiler folds a product
// and its conversion to float16 into one v_fma_mixlo_f16, which rounds once where the rule rounds twice — the tests show it.)
__host__ __device__ inline float mix_f32_result(float f) {
#ifdef __HIP_DEVICE_COMPILE__
    asm("" : "+v"(f));
#endif
    return f;
}
template <int DT> __host__ __device__ inline uint32_t mix_rule(uint32_t self, uint32_t partner, float ws, float wp) {
    const float a = mix_load<DT>(mix_store<DT>(mix_f32_result(mix_load<DT>(partner) * wp)));
    const float b = mix_load<DT>(mix_store<DT>(mix_f32_result(mix_load<DT>(self) * ws)));
    return mix_store<DT>(mix_f32_result(a + b));
}
// ... with the type known at run time only (a lone element; the host twin)
__host__ __device__ inline uint32_t mix_rule(uint32_t self, uint32_t partner, float ws, float wp, int dtype) {
    return dtype == kDtypeF32 ? mix_rule<kDtypeF32>(self, partner, ws, wp) : dtype == kDtypeF16 ? mix_rule<kDtypeF16>(self, partner, ws, wp)
                                                                                                 : mix_rule<kDtypeBF16>(self, partner, ws, wp);
}

// a box (x, y, w, h) of a canvas as intervals of lines and of offsets inside a line (see above)
struct MixBox {
    uint32_t len, lines;        // elements per line; lines per plane
    uint32_t l0, ln, o0, on;
};
__host__ __device__ inline MixBox mix_box(const EraseCanvas &k, int x, int y, int w, int h) {
    const bool rows = (k.layout & 1) != 0;
    const uint32_t group = k.layout >= 2 ? 1u : (uint32_t)k.C;
    MixBox b;
    b.len = (uint32_t)(rows ? k.ow : k.oh) * group;
    b.lines = (uint32_t)(rows ? k.oh : k.ow);
    b.l0 = (uint32_t)(rows ? y : x); b.ln = (uint32_t)(rows ? h : w);
    b.o0 = (uint32_t)(rows ? x : y) * group; b.on = (uint32_t)(rows ? w : h) * group;
    return b;
}
__host__ __device__ inline bool mix_inside(const MixBox &b, uint32_t line, uint32_t off) { return line - b.l0 < b.ln && off - b.o0 < b.on; }
// line (within its plane) and offset of element e of a slot: the one division, made once per vector run or lone element
__host__ __device__ inline void mix_locate(const MixBox &b, int64_t e, uint32_t *line, uint32_t *off) {
    uint32_t r;                             // (the line counted through the planes: below 3 * 65535)
    if (e < ((int64_t)1 << 32)) { r = (uint32_t)e / b.len; *off = (uint32_t)e - r * b.len; }
    else { r = (uint32_t)((uint64_t)e / b.len); *off = (uint32_t)((uint64_t)e - (uint64_t)r * b.len); }
    if (r >= b.lines) r -= b.lines;         // (at most three planes)
    if (r >= b.lines) r -= b.lines;
    *line = r;
}

// elements in a slot
__host__ __device__ inline int64_t mix_slot_elems(const EraseCanvas &k) { return (int64_t)k.ow * k.oh * k.C; }

struct MixArgs {
    const void *src;
    void *dst;
    const DevMixOp *ops;
    EraseCanvas canvas;
    int32_t dtype, n_outputs;
    int32_t chunks;             // workgroup-sized pieces per slot
};
constexpr int kMixUnroll = 4;                               // 16-byte vectors per lane and piece
constexpr int kMixChunkVecs = 256 * kMixUnroll;             // ... per piece
// esize: 1, 2 or 4 bytes per element; a.chunks is filled in
hipError_t launch_mix(hipStream_t stream, MixArgs a, int esize);

}  // namespace mj
