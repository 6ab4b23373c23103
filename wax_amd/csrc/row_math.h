// row_math.h — the exact f32 distance of one row, defined ONCE (device side; included by the .hip kernel units only).
//
// An exact distance has the same bits whichever kernel computes it: the single-query scan, the
// multi-query scan, the batched re-scores and the mirror scan's finish all call the definitions below. A row's
// summation order is fixed by (GROUP, LOADS) alone, and (dims -> GROUP) is the one table at the end of this file.
// What a kernel keeps for itself is its load scheduling: rows in flight, non-temporal or plain loads, where the query
// comes from. Everything between "registers hold q and v" and "d" is here.
#pragma once
#include <type_traits>

#include "kernels.h"
#include "topk.h"

namespace wax {

typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { M_COS = WAX_HIP_METRIC_COSINE, M_DOT = WAX_HIP_METRIC_DOT, M_L2 = WAX_HIP_METRIC_L2 };

// a norm at or below this scores 0 under cosine (CosineDistance.metal:323 `sqrt(m) > 1e-6`)
constexpr float COS_NORM_FLOOR = 1e-6f;

// a3 + a6 (distance side): CosineDistance.metal:321-325 rule `sqrt(m) > 1e-6 ? dot/sqrt(m) : 0`,
// extended to the true cosine the CPU path computes (divide by ||q|| as well;
// SURVEY.md §7 "Query-norm semantics"); dot / l2 use USearch's ip / l2sq distances
// (VectorMetric.swift:21-30). NaN -> +inf so it sorts last and is dropped on the host
// like MetalVectorEngine.swift:597; "+ 0.0f" folds -0 into +0.
template <int METRIC>
__device__ inline float finish_distance(float acc, float nrm, float q_norm) {
    float d;
    if (METRIC == M_COS) {
        const float vn = sqrtf(nrm);
        const float sim = (vn > COS_NORM_FLOOR && q_norm > COS_NORM_FLOOR) ? acc / (vn * q_norm) : 0.0f;
        d = 1.0f - sim;
    } else if (METRIC == M_DOT) {
        d = 1.0f - acc;
    } else {
        d = acc;
    }
    d = (d != d) ? __builtin_inff() : d;
    return d + 0.0f;
}

// one step of the per-component fma chains: q.v (cosine, dot) or |q - v|^2 (l2) into acc, |v|^2 into nrm
template <int METRIC>
__device__ inline void accumulate_dot(const f32x4& q, const f32x4& v, f32x4& acc) {
    if (METRIC == M_L2) {
        const f32x4 e = q - v;
        acc = __builtin_elementwise_fma(e, e, acc);
    } else {
        acc = __builtin_elementwise_fma(q, v, acc);
    }
}
__device__ inline void accumulate_norm(const f32x4& v, f32x4& nrm) { nrm = __builtin_elementwise_fma(v, v, nrm); }
template <int METRIC>
__device__ inline void accumulate(const f32x4& q, const f32x4& v, f32x4& acc, f32x4& nrm) {
    accumulate_dot<METRIC>(q, v, acc);
    if (METRIC == M_COS) accumulate_norm(v, nrm);
}

__device__ inline float hsum(const f32x4& a) { return (a.x + a.y) + (a.z + a.w); }

// ---------------------------------------------------------------------------
// The end of every row: a lane's chains -> the GROUP lanes' sums (valid in the group's LAST lane) -> the distance.
template <int GROUP, int METRIC>
__device__ inline float finish_row(const f32x4& acc, const f32x4& nrm, float q_norm) {
    const float s = group_sum<GROUP>(hsum(acc));
    float m = 0.f;
    if (METRIC == M_COS) m = group_sum<GROUP>(hsum(nrm));
    return finish_distance<METRIC>(s, m, q_norm);
}

// One row, compile-time dims: GROUP lanes per row, lane g holds the row's float4s g, g + GROUP, ... in v (the query's in q).
// (scan_body and scan_multi_kernel, the streaming kernels, spell this loop out: handing a function their register arrays moves
// their loads in the generated code. They call the same accumulate / finish_row.)
template <int GROUP, int LOADS, int METRIC>
__device__ inline float row_distance(const f32x4 (&q)[LOADS], const f32x4 (&v)[LOADS], float q_norm) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, nrm = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < LOADS; ++j) accumulate<METRIC>(q[j], v[j], acc, nrm);
    return finish_row<GROUP, METRIC>(acc, nrm, q_norm);
}

// One row, any dims (D not in the table, D % 4 != 0 included): the whole wave on the row, lanes striding it; float4 steps
// when D % 4 == 0, else one element per lane and step in component x. Valid in lane 63.
template <int METRIC>
__device__ inline float generic_row_distance(const float* row, const float* query, uint32_t D, int lane, float q_norm) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, nrm = {0.f, 0.f, 0.f, 0.f};
    if ((D & 3u) == 0) {
        const f32x4* row4 = reinterpret_cast<const f32x4*>(row);
        const f32x4* q4 = reinterpret_cast<const f32x4*>(query);
        for (uint32_t c = lane; c < (D >> 2); c += WAVE) accumulate<METRIC>(q4[c], row4[c], acc, nrm);
    } else {
        for (uint32_t c = lane; c < D; c += WAVE) {
            const f32x4 qq = {query[c], 0.f, 0.f, 0.f};
            const f32x4 vv = {row[c], 0.f, 0.f, 0.f};
            accumulate<METRIC>(qq, vv, acc, nrm);
        }
    }
    return finish_row<64, METRIC>(acc, nrm, q_norm);
}

// sum x^2 of one row exactly as the scan of a G-lanes-per-row dimension forms it (G = 64: the any-dims form too), read from memory
// by the whole wave: every aligned group of G lanes computes the same row, the total is handed to every lane. These are the bits
// of the `m` finish_distance tests against COS_NORM_FLOOR, so a row is a zero row in the bf16 mirror exactly when the scan scores it 0.
template <int G>
__device__ inline float scan_order_norm2(const float* __restrict__ row, uint32_t dims, int lane) {
    f32x4 nrm = {0.f, 0.f, 0.f, 0.f};
    const uint32_t gl = (uint32_t)lane % G;
    if ((dims & 3u) == 0) {
        const f32x4* row4 = reinterpret_cast<const f32x4*>(row);
        for (uint32_t c = gl; c < (dims >> 2); c += G) accumulate_norm(row4[c], nrm);
    } else {
        for (uint32_t c = gl; c < dims; c += G) {
            const f32x4 v = {row[c], 0.f, 0.f, 0.f};
            accumulate_norm(v, nrm);
        }
    }
    const float m = group_sum<G>(hsum(nrm));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 63));
}

// ---------------------------------------------------------------------------
// THE table: lanes per row at every specialised dimension (D4 = dims / 4 float4s per row, LOADS = D4 / GROUP per lane).
// Speed knobs (rows in flight, load flavour) live with the kernels; they never change a bit.
template <int DIMS_, int GROUP_>
struct ScanShapeOf {
    static constexpr int DIMS = DIMS_, D4 = DIMS_ / 4, GROUP = GROUP_, LOADS = D4 / GROUP_;
    static_assert(DIMS_ % 4 == 0 && D4 % GROUP_ == 0, "GROUP must divide D4");
};
template <int DIMS> struct ScanShape;
template <> struct ScanShape<64> : ScanShapeOf<64, 16> {};
template <> struct ScanShape<128> : ScanShapeOf<128, 32> {};
template <> struct ScanShape<256> : ScanShapeOf<256, 64> {};
template <> struct ScanShape<384> : ScanShapeOf<384, 32> {};
template <> struct ScanShape<512> : ScanShapeOf<512, 64> {};
template <> struct ScanShape<768> : ScanShapeOf<768, 64> {};
template <> struct ScanShape<1024> : ScanShapeOf<1024, 64> {};
template <> struct ScanShape<1536> : ScanShapeOf<1536, 64> {};

template <int... DIMS> struct DimList {};
using ScanDims = DimList<64, 128, 256, 384, 512, 768, 1024, 1536>;   // every specialised dimension

// Host-side visitors: f(ScanShape<dims>{}) if `dims` is in the list (a path that serves a subset names it), else `none`;
// f(std::integral_constant<int, metric>{}) likewise.
template <int... DIMS, typename F, typename R>
inline R with_scan_shape(DimList<DIMS...>, uint32_t dims, F&& f, R none) {
    (void)((dims == (uint32_t)DIMS ? (none = f(ScanShape<DIMS>{}), true) : false) || ...);
    return none;
}
template <typename F, typename R>
inline R with_scan_shape(uint32_t dims, F&& f, R none) { return with_scan_shape(ScanDims{}, dims, f, none); }

template <int... METRICS, typename F, typename R>
inline R with_metric_in(int metric, F&& f, R none) {
    (void)((metric == METRICS ? (none = f(std::integral_constant<int, METRICS>{}), true) : false) || ...);
    return none;
}
template <typename F, typename R>
inline R with_metric(int metric, F&& f, R none) { return with_metric_in<M_COS, M_DOT, M_L2>(metric, f, none); }

template <int... DIMS>
inline bool in_dim_list(DimList<DIMS...>, uint32_t dims) { return ((dims == (uint32_t)DIMS) || ...); }

// lanes per row of the scan at `dims`; 0 = not specialised (the any-dims form: the whole wave)
inline int scan_group_lanes(uint32_t dims) {
    return with_scan_shape(dims, [](auto s) { return decltype(s)::GROUP; }, 0);
}

}  // namespace wax
