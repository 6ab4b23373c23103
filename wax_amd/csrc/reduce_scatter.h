// reduce_scatter.h — group_sum<GROUP>'s summation tree as a reduce-scatter over the lanes of a row (device only).
//
// A wave that scores MS_U row-groups against MS_NQ queries holds MS_M lane-private partial sums. Summing each with group_sum<> costs
// 5-6 DPP adds in all 64 lanes for one useful lane; the levels below halve the values a lane holds instead, adding the SAME pairs
// (IEEE addition is commutative, so the bits are group_sum's), and every lane ends with complete sums of DIFFERENT (query, row) pairs.
// Used by the streaming multi-query scan (multiscan.hip) and the resident batched search (batch_resident.hip).
#pragma once
#include "common.h"

namespace wax {

constexpr int MS_NQ = 16;      // queries per pass (a shorter last group is padded with idle slots)
constexpr int MS_U = 4;        // row-groups a wave holds in registers per chunk
constexpr int MS_M = MS_NQ * MS_U;   // partial sums per lane per chunk: value m = u * 16 + q

template <int CTRL>
__device__ inline float ms_dpp_move(float v) {   // v of the lane the DPP pattern names (every lane has a source)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

// One halving level of the reduce-scatter: n values per lane -> n / 2. Of every pair (v[2i], v[2i+1]) a lane KEEPS one
// (sel: the odd one) and SENDS the other to its partner lane, which keeps the opposite one: out[i] = kept + partner's.
// Both lanes of a pair end up with the sum of the SAME two partial sums group_sum<> adds at this level (it adds them in
// both lanes and keeps both copies) — IEEE addition is commutative, so the bits are scan_kernel's. CTRL names the partner:
// xor 1, xor 2, 7 - i (row_half_mirror), 15 - i (row_mirror), exactly group_sum's patterns.
template <int CTRL, int N>
__device__ inline void ms_halve(float (&v)[MS_M], bool sel) {
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
        const float a = v[2 * i], b = v[2 * i + 1];
        const float keep = sel ? b : a, send = sel ? a : b;
        v[i] = keep + ms_dpp_move<CTRL>(send);
    }
}
// Levels 5 / 6 (16-lane rows, 32-lane halves): v_permlane16_swap / v_permlane32_swap exchange the odd rows (upper half) of
// the first operand with the even rows (lower half) of the second, so even rows hold both parts of v[2i], odd rows both
// parts of v[2i+1]: one swap + one add per output, no select.
template <int N>
__device__ inline void ms_halve_rows16(float (&v)[MS_M]) {
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[2 * i]), __float_as_uint(v[2 * i + 1]), false, false);
        v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
}
template <int N>
__device__ inline void ms_halve_rows32(float (&v)[MS_M]) {
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[2 * i]), __float_as_uint(v[2 * i + 1]), false, false);
        v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
}

}  // namespace wax
