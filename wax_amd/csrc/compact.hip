// compact.hip — order-preserving removal of MANY rows in one pass (wax_hip_remove_batch).
//
// Input: the ascending, duplicate-free list rem[0..m) of removed rows. A surviving row r moves to r - rank(r), rank(r) = entries of
// rem below r. Up to four per-row arrays take the same map: the f32 store, the frame ids, and (rows below the mirror's fill only)
// the bf16 mirror and its norms.
//
// The move is in place and every destination lies at or below its source, so the only hazard is a workgroup overwriting rows that
// another has not read yet. It is resolved by launch order on one stream, never by waiting inside a kernel: the host (engine.hip,
// api_store.inc) cuts [first surviving row behind rem[0], count) into windows of source rows, ascending, and one launch of the kernel
// below moves one window — into the bounce buffer when the window's destination range can reach into the window itself (a copy
// behind it on the same stream puts the rows in place: the window has been consumed by then), or straight to its destination
// once the shift rank(w0) has reached the window's length (source and destination ranges are disjoint). Either way a launch never
// reads a byte that the same launch writes, which is what the __restrict__ qualifiers below say.
//
// Kernel shape: a workgroup of four waves owns 64 consecutive source rows. Every wave finds the chunk's place in `rem` by one
// binary search over the window's slice of the list, builds the chunk's 64-bit "removed" mask from the (at most 64) entries that
// follow, and from then on a row's rank is a popcount — no search per row. Wide rows (the vectors) are moved one row per wave,
// 16 bytes per lane (4 or 2 bytes where the row is not a multiple of 16), four rows in flight per wave; narrow rows (ids, norms) one
// row per lane. The source is streamed with non-temporal loads on large windows; stores are ordinary (the bounce buffer is meant
// to stay in the last-level cache until the copy behind the launch has read it).
#include "kernels.h"

namespace wax {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kChunkRows = 64;      // = one wave's ballot width
constexpr int kRowsInFlight = 4;    // rows a wave loads before it stores

template <bool NT, typename T>
__device__ inline T ld(const T* p) {
    if (NT) return __builtin_nontemporal_load(p);
    return *p;
}

// 64-bit OR over the wave
__device__ inline uint64_t wave_or(uint64_t v) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
    for (int s = 1; s < WAVE; s <<= 1) {
        lo |= (uint32_t)__shfl_xor((int)lo, s, WAVE);
        hi |= (uint32_t)__shfl_xor((int)hi, s, WAVE);
    }
    return ((uint64_t)hi << 32) | lo;
}

// one wide array, rows [c0, c0 + 64) of it, rows t = wave, wave + 4, ... — T is the lane's unit (16 or 4 bytes)
template <bool NT, typename T>
__device__ inline void move_wide(const RowCompactArray& a, uint32_t c0, uint32_t c_end, uint64_t mask, uint32_t rank0, uint32_t dst0,
                                 int wave, int lane) {
    const uint32_t units = a.row_bytes / (uint32_t)sizeof(T);
    const T* __restrict__ src = reinterpret_cast<const T*>(a.src);
    T* __restrict__ out = reinterpret_cast<T*>(a.out);
    const uint32_t end = c_end < a.limit ? c_end : a.limit;
    const uint32_t n_here = end > c0 ? end - c0 : 0;
    // this wave's rows: 16 consecutive ones (a contiguous 16-row stretch of the source), taken kRowsInFlight at a time
    constexpr int kPerWave = kChunkRows / SCAN_WAVES;
    for (int g = 0; g < kPerWave; g += kRowsInFlight) {
        uint64_t s_off[kRowsInFlight], d_off[kRowsInFlight];
        bool live[kRowsInFlight];
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) {
            const int t = wave * kPerWave + g + u;
            const uint32_t r = c0 + (uint32_t)t;
            live[u] = (uint32_t)t < n_here && !((mask >> t) & 1ull);
            const uint32_t below = rank0 + (uint32_t)__popcll(mask & ((1ull << t) - 1ull));
            s_off[u] = (uint64_t)r * units;
            d_off[u] = (uint64_t)(r - below - dst0) * units;   // (only read when live: r - below >= dst0 then)
        }
        for (uint32_t col = (uint32_t)lane; col < units; col += WAVE) {
            T v[kRowsInFlight];
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u)
                if (live[u]) v[u] = ld<NT>(src + s_off[u] + col);
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u)
                if (live[u]) out[d_off[u] + col] = v[u];
        }
    }
}

// one narrow array (a row is one T): lane t moves row c0 + t
template <typename T>
__device__ inline void move_narrow(const RowCompactArray& a, uint32_t c0, uint32_t c_end, uint64_t mask, uint32_t rank0, uint32_t dst0,
                                   int lane) {
    const T* __restrict__ src = reinterpret_cast<const T*>(a.src);
    T* __restrict__ out = reinterpret_cast<T*>(a.out);
    const uint32_t end = c_end < a.limit ? c_end : a.limit;
    const uint32_t n_here = end > c0 ? end - c0 : 0;
    const uint32_t r = c0 + (uint32_t)lane;
    if ((uint32_t)lane >= n_here || ((mask >> lane) & 1ull)) return;
    const uint32_t below = rank0 + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    out[r - below - dst0] = src[r];
}

template <bool NT>
__global__ __launch_bounds__(SCAN_THREADS) void compact_rows_kernel(const RowCompactArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)), lane = (int)(threadIdx.x % WAVE);
    const uint32_t c0 = a.w0 + blockIdx.x * (uint32_t)kChunkRows;
    if (c0 >= a.w1) return;
    const uint32_t c_end = a.w1 - c0 < (uint32_t)kChunkRows ? a.w1 : c0 + (uint32_t)kChunkRows;
    // rank(c0): lower bound of c0 in rem[p0, p1) — the window's slice of the list (uniform: scalar loads)
    uint32_t lo = a.p0, hi = a.p1;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a.rem[mid] < c0) lo = mid + 1; else hi = mid;
    }
    const uint32_t rank0 = lo;
    // the chunk's removed rows are among the next 64 entries (ascending, distinct)
    uint64_t bit = 0;
    if (rank0 + (uint32_t)lane < a.p1) {
        const uint32_t v = a.rem[rank0 + (uint32_t)lane];
        if (v < c_end) bit = 1ull << (v - c0);
    }
    const uint64_t mask = wave_or(bit);
    for (int i = 0; i < a.n_arrays; ++i) {
        const RowCompactArray& arr = a.arr[i];
        if (arr.row_bytes == 8) {
            if (wave == (i & 3)) move_narrow<uint64_t>(arr, c0, c_end, mask, rank0, a.dst0, lane);
        } else if (arr.row_bytes == 4) {
            if (wave == (i & 3)) move_narrow<uint32_t>(arr, c0, c_end, mask, rank0, a.dst0, lane);
        } else if ((arr.row_bytes & 15u) == 0) {
            move_wide<NT, f32x4>(arr, c0, c_end, mask, rank0, a.dst0, wave, lane);
        } else if ((arr.row_bytes & 3u) == 0) {
            move_wide<NT, uint32_t>(arr, c0, c_end, mask, rank0, a.dst0, wave, lane);
        } else {
            move_wide<NT, uint16_t>(arr, c0, c_end, mask, rank0, a.dst0, wave, lane);   // bf16 rows of an odd dimension
        }
    }
}

}  // namespace

hipError_t launch_compact_rows(const RowCompactArgs& a, bool nontemporal, hipStream_t st) {
    if (a.w1 <= a.w0 || a.n_arrays <= 0) return hipSuccess;
    if (a.n_arrays > kCompactMaxArrays || a.p0 > a.p1) return hipErrorInvalidValue;
    for (int i = 0; i < a.n_arrays; ++i)
        if (a.arr[i].row_bytes == 0 || (a.arr[i].row_bytes & 1u)) return hipErrorInvalidValue;   // f32 / bf16 / u64 rows: always even
    const uint32_t grid = (a.w1 - a.w0 + (uint32_t)kChunkRows - 1) / (uint32_t)kChunkRows;
    if (nontemporal) hipLaunchKernelGGL((compact_rows_kernel<true>), dim3(grid), dim3(SCAN_THREADS), 0, st, a);
    else hipLaunchKernelGGL((compact_rows_kernel<false>), dim3(grid), dim3(SCAN_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace wax
