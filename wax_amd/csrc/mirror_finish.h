// mirror_finish.h — the finish of ONE query by one workgroup, behind a pass over either mirror (device code; mirror_scan.hip and
// mirror8_scan.hip include it). The four finish kernels say where the query's MirrorScanArgs and floats are (the kernel arguments for
// a lone query, MirrorMember for a member of a group) and which EPS the certificate subtracts:
//   struct EPS { template <int DIMS, int METRIC> static __device__ float eps(const MirrorScanArgs& a); };
#pragma once
#include "kernels.h"
#include "row_math.h"
#include "topk.h"

namespace wax {

// The bf16 mirror's eps: batch_prep_kernel's bound (batch.hip) with the query-side rounding term gone — the query is not rounded. With
// x_v the f32 row that was rounded (normalised for cosine) and v~ its bf16 rounding, |q.v~ - q.x_v| <= ||q|| ||v~ - x_v||, bounded by
// ||q|| max_rows ||v~ - x_v|| (measured when the mirror was converted, + 0.1 % for its f32 accumulation); the f32 sums on
// either side and the normalisations stay inside 3 D 2^-24 of ||q|| max||v||; the exact distance carries ~1e-6 of its own.
// Without a measurement: the worst case of one rounded operand is below the batched path's two-operand constant, kept as is.
// Cosine divides by ||q||, so both norms are 1 there.
struct Bf16Eps {
    template <int DIMS, int METRIC>
    static __device__ __forceinline__ float eps(const MirrorScanArgs& a) {
        const unsigned int* mb = a.max_bits;
        const float max_norm = __uint_as_float(mb[0]);
        const float max_row_err = a.use_measured ? __uint_as_float(mb[1]) : 0.f;
        const double qn_d = METRIC == M_COS ? 1.0 + 1e-6 : (double)a.q_norm;
        const double vn_d = METRIC == M_COS ? 1.0 + 1e-6 : (double)max_norm;
        const double u = 0.0078125 * (1.0 + 1.0 / 512.0) + (double)DIMS * 5.97e-8 + 1e-6;
        double dot_err = u * qn_d * vn_d * 1.001;
        if (max_row_err > 0.f) {
            const double measured = qn_d * (double)max_row_err * 1.001 + 3.0 * (double)DIMS * 5.97e-8 * qn_d * vn_d;
            if (measured < dot_err) dot_err = measured;
        }
        const float eps = METRIC == M_COS ? (float)(dot_err + 3e-6) : (float)(dot_err + 1e-6 * (1.0 + qn_d * vn_d));
        return nextafterf(eps, __builtin_inff());             // the double -> float conversion may have rounded down
    }
};

template <int DIMS, int METRIC, class EPS>
__device__ __forceinline__ void mirror_finish(const MirrorScanArgs& a, const f32x4* q4) {
    constexpr int D4 = ScanShape<DIMS>::D4;
    constexpr int GROUP = ScanShape<DIMS>::GROUP;
    constexpr int LOADS = ScanShape<DIMS>::LOADS;
    constexpr int RPW = WAVE / GROUP;
    constexpr int ROWS_PER_PASS = RPW * SCAN_WAVES;
    constexpr int PASSES = MIRROR_KP / ROWS_PER_PASS;
    static_assert(MIRROR_KP % ROWS_PER_PASS == 0, "whole passes");
    static_assert(GATHER_CAP == 2 * MIRROR_KP && 2 * SCAN_WAVES * sizeof(int64_t) >= (1 + SCAN_WAVES) * sizeof(int), "the selection's buffers are (2)-(3)'s and the merge's");
    __shared__ int64_t approx[MIRROR_KP], work[2 * MIRROR_KP], xch[2 * SCAN_WAVES];
    int64_t* const exact = work;                  // (2), (3); until then `work` is the selection's gather buffer, and `xch` its control
                                                  // words before it is the merge's: gather_select leaves through a barrier on both ways out
    int64_t* const sorted = work + MIRROR_KP;
    const int t = (int)threadIdx.x;
    const int lane = lane_id();
    const int wave = t >> 6;

    // (1) the MIRROR_KP best approximate keys of the whole store: the lists' prefixes under a bound from their heads, sorted in LDS
    // (gather_select, topk.h); the k-way merge of the heads, whose answer that is, when they overflow the buffer
    if (a.lists <= SCAN_THREADS) {
        if (!gather_select<1>(a.partials, a.lists, MIRROR_KP, approx, work, reinterpret_cast<int*>(xch))) kway_merge<1>(a.partials, a.lists, MIRROR_KP, approx, xch);
    } else {
        if (!gather_select<2>(a.partials, a.lists, MIRROR_KP, approx, work, reinterpret_cast<int*>(xch))) kway_merge<2>(a.partials, a.lists, MIRROR_KP, approx, xch);
    }

    // (2) exact f32 re-score of those rows: row_distance (row_math.h) at the f32 scan's shape for this dimension
    const int sub = lane / GROUP, gl = lane % GROUP;
    f32x4 q[LOADS];
#pragma unroll
    for (int j = 0; j < LOADS; ++j) q[j] = q4[gl + j * GROUP];
    const f32x4* __restrict__ store4 = reinterpret_cast<const f32x4*>(a.store);
    f32x4 v[PASSES][LOADS];
    bool live[PASSES];
    uint32_t grow[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {   // every load of the wave in flight before the first product
        const int i = p * ROWS_PER_PASS + wave * RPW + sub;
        const int64_t key = approx[i];
        grow[p] = key_row(key);
        const uint32_t lrow = grow[p] - a.row_base;
        live[p] = key != KEY_PAD && lrow < a.n_rows;
        const f32x4* src = store4 + (size_t)(live[p] ? lrow : 0u) * D4 + gl;
#pragma unroll
        for (int j = 0; j < LOADS; ++j) v[p][j] = src[j * GROUP];
    }
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const float d = row_distance<GROUP, LOADS, METRIC>(q, v[p], a.q_norm);
        if (gl == GROUP - 1) exact[p * ROWS_PER_PASS + wave * RPW + sub] = live[p] ? make_key(d, grow[p]) : KEY_PAD;
    }
    __syncthreads();

    // (3) rank sort of the exact keys (unique rows; KEY_PAD ties broken by position)
    if (t < MIRROR_KP) {
        const int64_t key = exact[t];
        int rank = 0;
        for (int j = 0; j < MIRROR_KP; ++j) {
            const int64_t o = exact[j];
            rank += (o < key || (o == key && j < t)) ? 1 : 0;
        }
        sorted[rank] = key;
    }
    __syncthreads();

    // (4) the k best with frame ids
    for (int i = t; i < a.kpad; i += SCAN_THREADS) {
        wax_hip_hit h;
        h.key = (i < a.k) ? sorted[i] : KEY_PAD;
        h.frame_id = ID_PAD;
        if (h.key != KEY_PAD) {
            const uint32_t local = key_row(h.key) - a.row_base;
            h.frame_id = (a.ids != nullptr && local < a.n_rows) ? a.ids[local] : (uint64_t)key_row(h.key);
        }
        a.hits[i] = h;
    }
    // (5) the certificate: `approx` holds approximate distances (Bf16Eps) or lower bounds (a unit that supplies its own slack)
    if (t == 0) {
        const float eps = EPS::template eps<DIMS, METRIC>(a);
        const int64_t a_kp = approx[MIRROR_KP - 1], kth = sorted[a.k - 1];
        const float da = key_distance(a_kp), dk = key_distance(kth);
        const bool ok = a_kp != KEY_PAD && kth != KEY_PAD && __builtin_isfinite(da) && __builtin_isfinite(dk) &&
                        __builtin_isfinite(eps) && a.q_norm == a.q_norm && (da - eps > dk);   // strict: ties stay uncertified
        *a.certified = ok ? 1u : 0u;
    }
}

}  // namespace wax
