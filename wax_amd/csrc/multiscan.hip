// multiscan.hip — the exact f32 scan for SEVERAL queries in one pass over the store.
//
// Who needs it: the batched (bf16 MFMA) path answers a query exactly or not at all — a query whose exactness
// certificate fails (dense neighbourhoods: more rows inside the bf16 error band of the k-th neighbour than the candidate
// list holds; duplicated rows; an overflowed survivor segment) is re-run on the exact path. Until round 3 that was one
// scan_kernel launch per such query, serially: on clustered stores a 256-query batch went from 0.23 ms to ~10 ms. Here
// up to 16 of those queries share ONE stream of the f32 store: the rows a wave holds in registers (the same UNROLL x LOADS
// dwordx4 loads per lane as scan_kernel) are scored against every query of the group before the next chunk is
// fetched, so the HBM traffic of the fallback is rows x dims x 4 bytes per GROUP of queries instead of per query.
//
// Bit-identity with the single-query path is the point (results must equal nq calls of wax_hip_search): a row's
// distance is built from row_math.h's pieces at row_math.h's (dims -> GROUP) — lane g of a GROUP-lane group owns float4s
// g, g + GROUP, ..., one fma chain per component over j, hsum, finish_distance — with the DPP tree of group_sum<GROUP>
// replaced by a reduce-scatter that adds the same pairs (ms_halve). Only the loop order differs (queries inside rows).
//
// Layout per workgroup (4 waves, like scan_kernel):
//   * the group's queries sit in LDS as float4 [nq][D4] (a lane re-reads its LOADS float4s per query: conflict-free
//     ds_read_b128, the two half-waves of GROUP = 32 read the same addresses = broadcast), prefetched one query ahead;
//   * every wave keeps one WaveTopK-style list per query in LDS (CAP slots: a push offers at most 64 / GROUP
//     candidates, so CAP >= k + 64 / GROUP suffices — 64 slots for k <= 60) with its threshold and count beside it;
//     after warm-up a (row, query) pair costs one 64-bit compare, and the rare insert runs out of line;
//   * at the end the four lists of a query are rank-merged (topk.h) into partials[query][workgroup][k];
//     merge_keys_multi (kernels.hip) reduces them per query and attaches frame ids.
// VALU budget: ~35 instructions per (query, row-group) against ~950 cycles of HBM time per row-group and SIMD at
// 8 TB/s: about 12 queries ride on the stream for free, 16 cost ~1.3 passes — against 16 passes before.
#include "kernels.h"
#include "row_math.h"
#include "topk.h"

namespace wax {

typedef __attribute__((address_space(3))) f32x4 lds_f32x4m;

// Per-(wave, query) selection state in LDS.
struct MsState {
    int64_t tau;   // only keys < tau can still enter the query's top-k (this wave's view)
    int cnt;       // live candidates in the list
    int pad;
};

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

// The kernel. Per chunk a wave holds MS_U row-groups (64 / GROUP rows each) in registers and forms, for each of the 16
// queries, the lane-private partial dot products exactly as scan_kernel does (float4 fma chains over j, hsum). The
// cross-lane sums are where a one-query-at-a-time loop drowns: 5-6 DPP adds, the division of the cosine, the key and the
// threshold test for EVERY (query, row-group) pair, in all 64 lanes, for one useful lane — ~50 of ~80 VALU cycles per pair.
// Instead the 64 partial sums a lane holds per chunk go through a reduce-scatter over the GROUP lanes with the SAME
// summation tree (ms_halve): ~3 instructions per pair, and afterwards every lane owns complete sums of DIFFERENT
// (query, row) pairs — the distance, key and threshold test run once per 64 pairs instead of once per pair. ~37 VALU
// cycles per (query, row-group): 16 queries fit under the HBM time of the rows they share.
// Which pair a lane ends with: value m = u * 16 + q, level L keeps bit L-1 of m = the lane's selection bit s_L with
// s1 = b0^b2, s2 = b1^b2, s3 = b2^b3, s4 = b3 (b = lane bits; the XORs make mirror partners agree on the bits already
// fixed), s5 = b4, s6 = b5: q = s1 + 2 s2 + 4 s3 + 8 s4 is a per-lane constant, u comes from the higher bits.
//
// LISTED = true is the gather form of wax_hip_search_batch_filtered: workgroup blockIdx.x is work item blockIdx.x of a table
// (a.item_group -> a.groups[]): one share of the rows of ONE compact row list (a.rows + row_off, ascending, a device-side count),
// scored against the up to 16 queries that share that list. Position r of the list is row rows[r]; everything else — the loads
// of a row, the lane mapping, the arithmetic, the key row_base + row — is the full-store form's, so distances are the same bits.
//
// scan_multi_pooled_kernel is the many-stores form of wax_hip_search_many: the same work table, but a group (a.item_group -> pool[])
// names its OWN store — base pointer, row count, key base — and its rows are contiguous, as in the full-store form. One launch then
// scores every store's queries; a work item beyond its store's chunks (the shares are sized on the host) writes empty partial lists.
// MASKED = true is that form for wax_hip_search_many_predicate: a group may carry a row bitmap (PoolGroup::bitmap, written by
// attr_mask_pooled_kernel just before), and a row is offered only where its bit is set. The rows, the loads, the lane mapping and
// the arithmetic are the unmasked form's — a passing row's distance has the same bits — so the chunk's bits only gate the push.
// All kernels are the one body of multiscan_body.inc (included, not called: the existing forms keep their instructions).
template <int D4, int GROUP, int METRIC, int CAP, bool LISTED>
__global__ __launch_bounds__(SCAN_THREADS) void scan_multi_kernel(ScanMultiArgs a) {
    constexpr bool POOLED = false, MASKED = false;
    const PoolGroup* pool = nullptr;
#include "multiscan_body.inc"
}

template <int D4, int GROUP, int METRIC, int CAP, bool MASKED>
__global__ __launch_bounds__(SCAN_THREADS) void scan_multi_pooled_kernel(ScanPoolArgs p) {
    constexpr bool LISTED = false, POOLED = true;
    const ScanMultiArgs& a = p.a;
    const PoolGroup* pool = p.pool;
#include "multiscan_body.inc"
}

// ---------------------------------------------------------------------------
// launch side: every specialised dimension of row_math.h's table

size_t scan_multi_lds_bytes(uint32_t dims, int cap) {
    return (size_t)MS_NQ * dims * 4 + (size_t)SCAN_WAVES * MS_NQ * cap * 8 + (size_t)SCAN_WAVES * MS_NQ * sizeof(MsState) + (size_t)MS_NQ * 4 +
           (size_t)MS_NQ * SCAN_WAVES * 4 + 16;
}

bool scan_multi_dims(uint32_t dims) { return scan_group_lanes(dims) != 0; }

// A push offers at most 4 candidates to one list (the 4 lanes that share a query), so CAP >= k + 4.
int scan_multi_cap(uint32_t dims, int k) {
    if (scan_group_lanes(dims) == 0 || k < 1 || k > FUSED_MAX_K) return 0;
    return (k + 4 <= 64) ? 64 : 256;
}

// Queries per launch: 16, where the group's queries and lists fit in LDS (k > 60 needs 256-slot lists: 16 queries x 4 waves x
// 2 KB = 128 KB beside the query block — only the smaller dimensions).
uint32_t scan_multi_group(uint32_t dims, int k) {
    const int cap = scan_multi_cap(dims, k);
    if (cap == 0) return 0;
    return scan_multi_lds_bytes(dims, cap) <= 160 * 1024 ? (uint32_t)MS_NQ : 0u;
}

// rows a wave consumes per chunk (MS_U row-groups)
static int ms_rows_per_chunk(uint32_t dims) { return (WAVE / scan_group_lanes(dims)) * MS_U; }

int scan_multi_grid(uint32_t n_rows, uint32_t dims, int grid_cap) {
    if (grid_cap <= 0) grid_cap = 512;
    if (grid_cap > MAX_GRID_BLOCKS) grid_cap = MAX_GRID_BLOCKS;
    const uint64_t nchunks = ((uint64_t)n_rows + ms_rows_per_chunk(dims) - 1) / ms_rows_per_chunk(dims);
    const uint64_t max_waves = (uint64_t)grid_cap * SCAN_WAVES;
    uint64_t waves = nchunks;
    if (nchunks > max_waves) {   // balance the grid-stride loop (as scan_grid_for does)
        const uint64_t iters = (nchunks + max_waves - 1) / max_waves;
        waves = (nchunks + iters - 1) / iters;
    }
    uint64_t blocks = (waves + SCAN_WAVES - 1) / SCAN_WAVES;
    if (blocks < 1) blocks = 1;
    if (blocks > (uint64_t)grid_cap) blocks = grid_cap;
    return (int)blocks;
}

template <int D4, int GROUP, int METRIC, int CAP, bool LISTED>
static hipError_t ms_launch_one(const ScanMultiArgs& a, int grid, size_t smem, hipStream_t st) {
    static std::atomic<uint64_t> configured{0};   // per device (ensure_dynamic_lds)
    if (smem > 64 * 1024) {
        hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&scan_multi_kernel<D4, GROUP, METRIC, CAP, LISTED>), 160 * 1024, configured);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((scan_multi_kernel<D4, GROUP, METRIC, CAP, LISTED>), dim3(grid), dim3(SCAN_THREADS), smem, st, a);
    return hipGetLastError();
}

template <bool LISTED>
static hipError_t ms_dispatch(const ScanMultiArgs& a, int metric, int cap, int grid, size_t smem, hipStream_t st) {
    return with_scan_shape(a.dims, [&](auto s) {
        using S = decltype(s);
        return with_metric(metric, [&](auto m) {
            constexpr int METRIC = decltype(m)::value;
            return cap == 64 ? ms_launch_one<S::D4, S::GROUP, METRIC, 64, LISTED>(a, grid, smem, st)
                             : ms_launch_one<S::D4, S::GROUP, METRIC, 256, LISTED>(a, grid, smem, st);
        }, hipErrorInvalidValue);
    }, hipErrorInvalidValue);
}

hipError_t launch_scan_multi(const ScanMultiArgs& a, int metric, int grid_cap, hipStream_t st, int* out_grid) {
    const int cap = scan_multi_cap(a.dims, a.k);
    if (cap == 0 || a.nq == 0 || a.nq > (uint32_t)MS_NQ) return hipErrorInvalidValue;
    const size_t smem = scan_multi_lds_bytes(a.dims, cap);
    if (smem > 160 * 1024) return hipErrorInvalidValue;
    const int grid = scan_multi_grid(a.n_rows, a.dims, grid_cap);
    if (out_grid) *out_grid = grid;
    return ms_dispatch<false>(a, metric, cap, grid, smem, st);
}

uint32_t scan_multi_listed_items(uint64_t max_rows, uint32_t dims, int grid_cap) {
    if (scan_group_lanes(dims) == 0 || max_rows == 0) return 1;
    // ~8 chunks per wave: few enough workgroups that the per-workgroup query load and list merge stay small beside the rows
    const uint64_t per_wg = (uint64_t)ms_rows_per_chunk(dims) * SCAN_WAVES * 8;
    uint64_t w = (max_rows + per_wg - 1) / per_wg;
    if (grid_cap <= 0) grid_cap = 512;
    if (w > (uint64_t)grid_cap) w = (uint64_t)grid_cap;
    return w < 1 ? 1u : (uint32_t)w;
}

hipError_t launch_scan_multi_listed(const ScanMultiArgs& a, int metric, uint32_t n_items, hipStream_t st) {
    const int cap = scan_multi_cap(a.dims, a.k);
    if (cap == 0 || n_items == 0 || !a.rows || !a.row_counts || !a.groups || !a.item_group) return hipErrorInvalidValue;
    const size_t smem = scan_multi_lds_bytes(a.dims, cap);
    if (smem > 160 * 1024) return hipErrorInvalidValue;
    return ms_dispatch<true>(a, metric, cap, (int)n_items, smem, st);
}

// ---- the many-stores form (wax_hip_search_many) ----

// Work items of one (store, group) when the whole launch may have `share` of them: scan_multi_grid's balanced split under that cap.
uint32_t scan_multi_pooled_items(uint32_t n_rows, uint32_t dims, uint32_t share) {
    if (scan_group_lanes(dims) == 0 || n_rows == 0) return 1;
    return (uint32_t)scan_multi_grid(n_rows, dims, share < 1 ? 1 : (int)share);
}
uint64_t scan_multi_chunks(uint32_t n_rows, uint32_t dims) {
    if (scan_group_lanes(dims) == 0) return 0;
    return ((uint64_t)n_rows + ms_rows_per_chunk(dims) - 1) / ms_rows_per_chunk(dims);
}

template <int D4, int GROUP, int METRIC, int CAP, bool MASKED>
static hipError_t ms_launch_pooled(const ScanPoolArgs& p, int grid, size_t smem, hipStream_t st) {
    static std::atomic<uint64_t> configured{0};   // per device (ensure_dynamic_lds)
    if (smem > 64 * 1024) {
        hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&scan_multi_pooled_kernel<D4, GROUP, METRIC, CAP, MASKED>), 160 * 1024, configured);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((scan_multi_pooled_kernel<D4, GROUP, METRIC, CAP, MASKED>), dim3(grid), dim3(SCAN_THREADS), smem, st, p);
    return hipGetLastError();
}

template <bool MASKED>
static hipError_t ms_dispatch_pooled(const ScanMultiArgs& a, const PoolGroup* d_pool, int metric, uint32_t n_items, hipStream_t st) {
    const int cap = scan_multi_cap(a.dims, a.k);
    if (cap == 0 || n_items == 0 || !d_pool || !a.item_group || !a.queries || !a.qlist || !a.q_norm || !a.partials) return hipErrorInvalidValue;
    const size_t smem = scan_multi_lds_bytes(a.dims, cap);
    if (smem > 160 * 1024) return hipErrorInvalidValue;
    ScanPoolArgs p{a, d_pool};
    return with_scan_shape(a.dims, [&](auto s) {
        using S = decltype(s);
        return with_metric(metric, [&](auto m) {
            constexpr int METRIC = decltype(m)::value;
            return cap == 64 ? ms_launch_pooled<S::D4, S::GROUP, METRIC, 64, MASKED>(p, (int)n_items, smem, st)
                             : ms_launch_pooled<S::D4, S::GROUP, METRIC, 256, MASKED>(p, (int)n_items, smem, st);
        }, hipErrorInvalidValue);
    }, hipErrorInvalidValue);
}

hipError_t launch_scan_multi_pooled(const ScanMultiArgs& a, const PoolGroup* d_pool, int metric, uint32_t n_items, hipStream_t st) {
    return ms_dispatch_pooled<false>(a, d_pool, metric, n_items, st);
}
hipError_t launch_scan_multi_pooled_masked(const ScanMultiArgs& a, const PoolGroup* d_pool, int metric, uint32_t n_items, hipStream_t st) {
    return ms_dispatch_pooled<true>(a, d_pool, metric, n_items, st);
}

}  // namespace wax
