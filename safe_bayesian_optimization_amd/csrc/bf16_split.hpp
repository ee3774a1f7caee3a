// bf16_split.hpp -- the split of an f32 value into three bf16 pieces,
// v = v0 + v1 + v2 (+ a remainder below 2^-24 |v|): v0 = bf16(v), v1 =
// bf16(v - v0), v2 = bf16((v - v0) - v1), every conversion one round to
// nearest even (v_cvt_pk_bf16_f32) and every subtraction exact in f32.
//
// One definition for the three units that multiply split operands on the bf16
// matrix cores: the split sweep's operand and K* (predict_x3_rowhalf.hpp), the
// Cholesky's outer panels (chol_x3.hip) and the tile norms (operand.hip),
// whose bounds are about the sweep's pieces and so must cut them identically.
// tests/plan_model.py models this split on the host.
//
// The vector types below carry a pair into the conversion and nothing else:
// no f32 arithmetic is vector-typed, so a unit built without packed f32 VALU
// (predict_x3) stays so.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace sbo {
namespace bf16s {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// two f32 -> one dword of two bf16 (element 0 low), round to nearest even
__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
// the two bf16 of a dword as f32
__device__ __forceinline__ float lo_f32(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float hi_f32(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// v = v0 + v1 + v2 for a pair of values (element 0 in the low halves)
__device__ __forceinline__ void split3(float a, float b, uint32_t &w0, uint32_t &w1, uint32_t &w2) {
    w0 = pk_bf16(a, b);
    const float ra = a - lo_f32(w0), rb = b - hi_f32(w0);
    w1 = pk_bf16(ra, rb);
    w2 = pk_bf16(ra - lo_f32(w1), rb - hi_f32(w1));
}

// the same for one value, the pieces as f32 (the pair's conversion with a zero partner)
__device__ __forceinline__ float bf16_rn(float a) { return lo_f32(pk_bf16(a, 0.0f)); }
__device__ __forceinline__ void split3(float x, float &a0, float &a1, float &a2) {
    a0 = bf16_rn(x);
    const float r1 = x - a0;
    a1 = bf16_rn(r1);
    a2 = bf16_rn(r1 - a1);
}

}  // namespace bf16s
}  // namespace sbo
