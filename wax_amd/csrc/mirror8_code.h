// mirror8_code.h — the arithmetic of a pass over the 8-bit code mirror, for every kernel that scores its codes on the matrix pipe
// (device code; mirror8_scan.hip's code8_pass at 384 / 768 dimensions and mirror8_dims.hip's at 512 / 1 024 / 1 536 include it): the
// query's three digit planes, and the one float epilogue from the exact integer plane sums to a row's key. DESIGN 4.1, "Eight bits
// per element".
#pragma once
#include "kernels.h"
#include "mirror_pass.h"

namespace wax {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// the wave's maximum in every lane (the build kernel and the query's quantiser)
__device__ inline float wave_max64(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// The query as three balanced base-128 digits per element, exact by construction:
//   M = 63 * 16384 + 63 * 128 + 63, delta = max|q| / M, m_i = rint(q_i * (1 / delta)) clamped to [-M, M] (one division per wave, one
//   product per element: both rounded, 2^-23 |m_i| <= 1/8 between them), m_i = 16384 a_i + 128 b_i + c_i with every digit in
//   [-64, 63], so ||q^ - q|| <= delta sqrt(D) (1/2 + 1/8) <= 1.18e-5 ||q|| at 384-d whatever the elements; tests/mirror8_planes_ref.py
//   restates it and tests/test_mirror8_planes_cpu.py finds 5.7e-6 at most, inside delta sqrt(D) / 2 every time.
// A query with a non-finite element gets delta = NaN: every s is NaN, every key -inf, the 64th key is not finite and the finish
// refuses the certificate. The all-zero query — and one whose delta would be subnormal, max|q| < 1.3e-32, where 1 / delta leaves
// the f32 range — gets delta = 0 and digits 0 (s = 0, like the f32 sum to within 1e-30 ||v||).
constexpr int PLANE_M = 63 * 16384 + 63 * 128 + 63;

// delta of the query at q4: the whole wave reads it once
template <int DIMS>
__device__ __forceinline__ float query_delta(const f32x4* q4, int lane) {
    float amax = 0.f;
    bool bad = false;
#pragma unroll
    for (int c = 0; c < (DIMS / 4 + WAVE - 1) / WAVE; ++c) {
        const int idx = lane + c * WAVE;
        if (idx < DIMS / 4) {
            const f32x4 v = q4[idx];
            bad = bad || !__builtin_isfinite(v.x) || !__builtin_isfinite(v.y) || !__builtin_isfinite(v.z) || !__builtin_isfinite(v.w);
            amax = fmaxf(fmaxf(amax, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        }
    }
    amax = wave_max64(amax);
    const float delta = __fdiv_rn(amax, (float)PLANE_M);
    return __ballot(bad) != 0ull ? __builtin_nanf("") : delta >= 1.17549435e-38f ? delta : 0.f;
}

// digit `plane` (0: a, 1: b, 2: c, else 0) of the 16 elements at q, as the bytes of one MFMA operand
__device__ __forceinline__ i32x4 query_digits(const float* q, float inv_delta, int plane) {
    const f32x4* q4 = reinterpret_cast<const f32x4*>(q);
    i32x4 out;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const f32x4 v = q4[w];
        const float x[4] = {v.x, v.y, v.z, v.w};
        unsigned int word = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float t = x[j] * inv_delta;
            t = rintf(fminf(fmaxf(t, -(float)PLANE_M), (float)PLANE_M));
            const int m = (int)t;
            const int c = ((m + 64) & 127) - 64, m1 = (m - c) >> 7;
            const int b = ((m1 + 64) & 127) - 64, a = (m1 - b) >> 7;
            const int d = plane == 0 ? a : plane == 1 ? b : plane == 2 ? c : 0;
            word |= ((unsigned int)d & 0xffu) << (8 * j);
        }
        out[w] = (int)word;
    }
    return out;
}

// v's value in lane Q of every quad
template <int Q>
__device__ __forceinline__ float quad_bcast(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), Q * 0x55, 0xF, 0xF, true));
}

// The key of one row for one query, from the integer sum S = sum_i m_i code_i (as a float: exact or rounded by code8_sum), delta,
// the row's {scale, err} and the query's norm: the ONE float epilogue of every form of the pass.
template <int METRIC>
__device__ __forceinline__ float code8_key(float S, float delta, f32x2 meta, float inv_qn, float q_norm) {
    const float s = (delta * meta.x) * S;
    const float lb = METRIC == M_COS ? (1.0f - s * inv_qn) - meta.y : (1.0f - s) - q_norm * meta.y;
    return (lb != lb) ? -__builtin_inff() : lb;
}

// S from the three plane sums (each below 2^24 in magnitude: the conversions are exact); two roundings
__device__ __forceinline__ float code8_sum(float pa, float pb, float pc) {
    return __builtin_fmaf(16384.0f, pa, __builtin_fmaf(128.0f, pb, pc));
}

}  // namespace

}  // namespace wax
