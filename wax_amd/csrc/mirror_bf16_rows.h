// mirror_bf16_rows.h — the bf16 mirror as a row format of mirror_pass (mirror_pass.h; device code). mirror_scan.hip scans it under
// the cosine and dot keys; mirror_l2.hip derives the L2 format from it (the same vectors, the row's ||v||^2 beside them).
#pragma once
#include "mirror_pass.h"

namespace wax {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Three dwordx4 (24 bf16) per lane and row, 4 row groups in flight (3 x 4 dwordx4 loads per lane, as scan_kernel's 384-d form), no
// side data, the key an approximate distance.
struct Bf16Rows {
    using Vec = u32x4;
    struct Side {};
    static constexpr int UNROLL = 4;
    static __device__ __forceinline__ Side side(const Side*, uint32_t) { return {}; }
    // two bf16 in dword c -> two f32, exactly (element 2i is the low half)
    static __device__ __forceinline__ f32x2 part(const Vec& v, int c) {
        f32x2 r;
        r.x = __uint_as_float(v[c] << 16);
        r.y = __uint_as_float(v[c] & 0xffff0000u);
        return r;
    }
    static __device__ __forceinline__ float start(const f32x2 (&)[3][4]) { return 0.f; }
    template <int METRIC>
    static __device__ __forceinline__ float key(float s, Side, float inv_qn, float) {
        const float d = METRIC == M_COS ? 1.0f - s * inv_qn : 1.0f - s;
        return (d != d) ? __builtin_inff() : d;
    }
};

}  // namespace wax
