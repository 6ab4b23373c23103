// grouped.hip — device side of wax_hip_search_grouped (PhotoRAGOrchestrator.swift:264-317,
// VideoRAGOrchestrator.swift:273-417): the `limit` best GROUPS of rows by their best member, and the best members of each.
//
// Every row has a group slot (a dense number of its root id, kept by the host; no slot column = slot is the row). A key is
// make_key(distance, row) (common.h), so a slot's smallest key is its best row under the tie rule of every search route.
//
//   group_fill_kernel      a word array to one value: `best` to KEY_PAD in front of every scan, the answer block to its padding.
//   group_scan_kernel      scan_body's streaming loop (kernels.hip): the same loads, accumulate / finish_row of row_math.h, so a row's
//                          distance has the scan's bits. No LDS lists: the owner lane of a row that takes part writes its distance
//                          (when members are wanted) and offers its key to best[slot], one iteration behind the row's loads.
//   group_offer_kernel     the column route (dimensions outside the lane-shape table, "force_general"): the same offers from the
//                          distance column the scan's write-distance form leaves.
//   group_split_kernel     best[slot] -> the slot's distance as ordered bits, sign-extended to int64; an empty slot -> INT64_MAX.
//                          launch_timeline (timeline.hip) then selects the `limit` smallest (distance, root id) pairs under the
//                          exclusive bound INT64_MAX, sorted: groups by (distance ascending, root id ascending as unsigned).
//   group_mark_kernel      one lane per slot: its rank in the sorted answer by binary search (pairs are unique: one slot per root), or
//                          -1; a chosen slot's best key becomes its first member and its "previous pick".
//   group_round_kernel     one lane per row, per_group - 1 times: a row of a chosen slot whose key is greater than that slot's previous
//                          pick offers it to cur[rank] by the same atomic minimum.
//   group_advance_kernel   between rounds: cur -> the answer and the previous pick, cur re-armed.
//   group_ids_kernel       frame ids of the members' rows.
//
// Nothing here depends on the order in which workgroups run: a minimum is a minimum, and keys are distinct.
#include "kernels.h"
#include "row_math.h"
#include "topk.h"

// Diagnosis only ("where the time goes"): 2 = the product; 1 = the fused scan's pre-check loads without its atomics;
// 0 = no offer at all. Builds below 2 answer nothing: they exist to be timed under a kernel trace.
#ifndef WAX_GROUP_OFFER
#define WAX_GROUP_OFFER 2
#endif

namespace wax {

namespace {

constexpr uint32_t kGroupGrid = 1024;      // most workgroups of the per-row and per-slot kernels (grid-strided)

__device__ inline void offer_key(int64_t* cell, int64_t key) {
    // The load may be stale. A value only ever falls during the launch, so a stale read costs an unneeded atomic and never a missed one.
    if (key < *cell) (void)__hip_atomic_fetch_min(cell, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A row's offer to its slot. A distance that is not finite takes no part (wax_hip_search drops such rows on the host).
__device__ inline void group_offer(int64_t* best, uint32_t slot, uint32_t n_slots, float d, uint32_t row) {
    if (slot >= n_slots || !(__builtin_fabsf(d) < __builtin_inff())) return;
    offer_key(best + slot, make_key(d, row));
}

__device__ inline bool bitmap_bit(const uint32_t* bitmap, uint32_t row) {
    return bitmap == nullptr || ((bitmap[row >> 5] >> (row & 31u)) & 1u) != 0u;
}

}  // namespace

__global__ __launch_bounds__(256) void group_fill_kernel(int64_t* p, uint64_t n, int64_t value) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) p[i] = value;
}

static hipError_t fill_words(int64_t* p, uint64_t n, int64_t value, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255ull) / 256ull;
    hipLaunchKernelGGL(group_fill_kernel, dim3((uint32_t)(blocks < 2048ull ? blocks : 2048ull)), dim3(256), 0, st, p, n, value);
    return hipGetLastError();
}

hipError_t launch_group_fill(int64_t* best, uint64_t n, hipStream_t st) {
    if (best == nullptr && n != 0) return hipErrorInvalidValue;
    return fill_words(best, n, KEY_PAD, st);
}

template <bool NT>
__device__ inline f32x4 ld16g(const f32x4* p) {
    if (NT) return __builtin_nontemporal_load(p);
    return *p;
}

template <int D4, int GROUP, int METRIC, int UNROLL, bool NT>
__global__ __launch_bounds__(SCAN_THREADS) void group_scan_kernel(GroupScanArgs a) {
    constexpr int LOADS = D4 / GROUP;       // float4s per lane per row
    constexpr int RPW = WAVE / GROUP;       // rows per wave-wide load
    constexpr int RPC = RPW * UNROLL;       // rows per wave per iteration
    static_assert(D4 % GROUP == 0, "GROUP must divide D4");

    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const int sub = lane / GROUP;
    const int gl = lane % GROUP;
    const bool owner = (gl == GROUP - 1);
    const uint32_t n = a.n_rows;

    const f32x4* __restrict__ store4 = reinterpret_cast<const f32x4*>(a.store);
    const f32x4* __restrict__ q4 = reinterpret_cast<const f32x4*>(a.query);

    f32x4 q[LOADS];
#pragma unroll
    for (int j = 0; j < LOADS; ++j) q[j] = q4[gl + j * GROUP];

    const uint32_t nchunks = (n + RPC - 1) / RPC;
    const uint32_t gwave = blockIdx.x * SCAN_WAVES + wave;
    const uint32_t nwaves = gridDim.x * SCAN_WAVES;

    // The offers run ONE ITERATION BEHIND the rows. An offer is a chain of dependent memory operations (slot -> best[slot] -> atomic)
    // and a wave has nothing else to do while it waits: offered at the end of a row's own iteration — the first build — the chain stood
    // between two iterations' row loads and the kernel took 1.6 x scan_kernel's time, with the atomics compiled out as with them
    // (DESIGN 4.10). Here a row's slot is loaded beside its floats, its key and slot wait in registers, and the pre-check load of
    // best[slot] goes out in FRONT of the next iteration's row loads: vmcnt counts in order, so the wave can take the pre-check's
    // answer while those rows are still in flight.
    constexpr uint32_t NO_SLOT = 0xffffffffu;
    int64_t pkey[UNROLL];
    uint32_t pslot[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) { pkey[u] = KEY_PAD; pslot[u] = NO_SLOT; }

    for (uint32_t chunk = gwave; chunk < nchunks; chunk += nwaves) {
        const uint32_t rbase = chunk * RPC + sub;
#if WAX_GROUP_OFFER >= 1
        int64_t seen[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) seen[u] = pslot[u] != NO_SLOT ? a.best[pslot[u]] : INT64_MIN;
#endif
        f32x4 v[UNROLL][LOADS];
        uint32_t nslot[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const uint32_t r = rbase + u * RPW;
            const uint32_t rc = r < n ? r : n - 1;  // clamp: tail lanes re-read the last row, result discarded
            const f32x4* p = store4 + (size_t)rc * D4 + gl;
#pragma unroll
            for (int j = 0; j < LOADS; ++j) v[u][j] = ld16g<NT>(p + j * GROUP);
            const bool part = owner && r < n && bitmap_bit(a.bitmap, r);
            nslot[u] = part ? (a.slots != nullptr ? a.slots[r] : r) : NO_SLOT;
        }
#if WAX_GROUP_OFFER >= 1
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            // The load may be stale. A value only ever falls during the launch, so a stale read costs an unneeded atomic and never a missed one.
            if (pkey[u] < seen[u]) {
#if WAX_GROUP_OFFER >= 2
                (void)__hip_atomic_fetch_min(a.best + pslot[u], pkey[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
                asm volatile("" ::"v"(seen[u]));
#endif
            }
        }
#endif
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f}, nrm = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < LOADS; ++j) accumulate<METRIC>(q[j], v[u][j], acc, nrm);
            const float d = finish_row<GROUP, METRIC>(acc, nrm, a.q_norm);
            const uint32_t r = rbase + u * RPW;
            pslot[u] = NO_SLOT;
            if (nslot[u] != NO_SLOT) {                       // the owner lane of a row that takes part
                if (a.dist_out != nullptr) a.dist_out[r] = d;
                // a distance that is not finite takes no part (wax_hip_search drops such rows on the host)
                if (nslot[u] < a.n_slots && __builtin_fabsf(d) < __builtin_inff()) { pslot[u] = nslot[u]; pkey[u] = make_key(d, r); }
            }
        }
    }
#if WAX_GROUP_OFFER >= 2
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
        if (pslot[u] != NO_SLOT) offer_key(a.best + pslot[u], pkey[u]);   // the last iteration's offers
#endif
}

// Row groups in flight per wave: the f32 scan's at 384-d and 768-d, elsewhere its default rule. Speed only: the lanes per row fix the bits.
template <typename S>
static constexpr int group_unroll() {
    return S::DIMS == 384 ? 4 : S::DIMS == 768 ? 2 : (12 / S::LOADS < 1 ? 1 : (12 / S::LOADS > 4 ? 4 : 12 / S::LOADS));
}

bool group_scan_dims(uint32_t dims) { return scan_group_lanes(dims) != 0; }

hipError_t launch_group_scan(const GroupScanArgs& a, int metric, int grid_cap, hipStream_t st) {
    if (a.n_rows == 0 || a.store == nullptr || a.query == nullptr || a.best == nullptr || a.n_slots == 0) return hipErrorInvalidValue;
    if (a.slots == nullptr && a.n_slots < a.n_rows) return hipErrorInvalidValue;
    const int grid = scan_grid_for(a.n_rows, a.dims, 0, grid_cap);
    return with_scan_shape(a.dims, [&](auto s) {
        using S = decltype(s);
        constexpr int U = group_unroll<S>();
        return with_metric(metric, [&](auto m) {
            constexpr int M = decltype(m)::value;
            launch_kernel((group_scan_kernel<S::D4, S::GROUP, M, U, true>), dim3(grid), dim3(SCAN_THREADS), 0, st, a);
            return hipGetLastError();
        }, hipErrorInvalidValue);
    }, hipErrorInvalidValue);
}

__global__ __launch_bounds__(256) void group_offer_kernel(const float* __restrict__ dist, const uint32_t* __restrict__ slots,
                                                          const uint32_t* __restrict__ bitmap, uint32_t n_rows, uint32_t n_slots, int64_t* best) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < n_rows; r += (uint64_t)gridDim.x * 256u) {
        const uint32_t row = (uint32_t)r;
        if (!bitmap_bit(bitmap, row)) continue;
        group_offer(best, slots != nullptr ? slots[row] : row, n_slots, dist[row], row);
    }
}

static uint32_t row_grid(uint64_t n, uint32_t grid) {
    const uint64_t tiles = (n + 255ull) / 256ull;
    uint64_t g = grid != 0u ? grid : kGroupGrid;
    if (g > kGroupGrid) g = kGroupGrid;
    if (g > tiles) g = tiles;
    return (uint32_t)(g < 1ull ? 1ull : g);
}

hipError_t launch_group_offer(const float* dist, const uint32_t* slots, const uint32_t* bitmap, uint32_t n_rows, uint32_t n_slots,
                              int64_t* best, uint32_t grid, hipStream_t st) {
    if (n_rows == 0 || dist == nullptr || best == nullptr || n_slots == 0) return hipErrorInvalidValue;
    if (slots == nullptr && n_slots < n_rows) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_offer_kernel, dim3(row_grid(n_rows, grid)), dim3(256), 0, st, dist, slots, bitmap, n_rows, n_slots, best);
    return hipGetLastError();
}

// best -> the timeline's "timestamp" column: the distance's ordered bits (int32 order == float order), sign-extended.
__global__ __launch_bounds__(256) void group_split_kernel(const int64_t* __restrict__ best, uint32_t n_slots, int64_t* __restrict__ dist_col) {
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n_slots; s += (uint64_t)gridDim.x * 256u) {
        const int64_t k = best[s];
        dist_col[s] = k == KEY_PAD ? INT64_MAX : (int64_t)(int32_t)(k >> 32);
    }
}

// sorted[0 .. *count) = the chosen (distance, root) pairs ascending. A chosen slot finds itself; every other slot gets -1.
__global__ __launch_bounds__(256) void group_mark_kernel(const int64_t* __restrict__ best, const uint64_t* __restrict__ slot_root, uint32_t n_slots,
                                                         const uint64_t* __restrict__ sorted_root, const int64_t* __restrict__ sorted_dist,
                                                         const uint32_t* __restrict__ count, int32_t limit, int32_t per_group,
                                                         int32_t* __restrict__ rank_of_slot, int64_t* __restrict__ member_keys,
                                                         int64_t* __restrict__ prev) {
    uint32_t n = *count;
    if (n > (uint32_t)limit) n = (uint32_t)limit;
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n_slots; s += (uint64_t)gridDim.x * 256u) {
        const int64_t k = best[s];
        int32_t rank = -1;
        if (k != KEY_PAD) {
            const int64_t d = (int64_t)(int32_t)(k >> 32);
            const uint64_t root = slot_root != nullptr ? slot_root[s] : s;
            uint32_t lo = 0, hi = n;                             // the first pair that is not below (d, root)
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                const int64_t md = sorted_dist[mid];
                const uint64_t mr = sorted_root[mid];
                if (md < d || (md == d && mr < root)) lo = mid + 1u; else hi = mid;
            }
            if (lo < n && sorted_dist[lo] == d && sorted_root[lo] == root) rank = (int32_t)lo;
        }
        rank_of_slot[s] = rank;
        if (rank >= 0) {
            member_keys[(size_t)rank * per_group] = k;
            prev[rank] = k;
        }
    }
}

__global__ __launch_bounds__(256) void group_round_kernel(const float* __restrict__ dist, const uint32_t* __restrict__ slots,
                                                          const uint32_t* __restrict__ bitmap, uint32_t n_rows, uint32_t n_slots,
                                                          const int32_t* __restrict__ rank_of_slot, const int64_t* __restrict__ prev,
                                                          int32_t limit, int64_t* cur) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < n_rows; r += (uint64_t)gridDim.x * 256u) {
        const uint32_t row = (uint32_t)r;
        if (!bitmap_bit(bitmap, row)) continue;
        const uint32_t slot = slots != nullptr ? slots[row] : row;
        if (slot >= n_slots) continue;
        const int32_t rank = rank_of_slot[slot];
        if (rank < 0 || rank >= limit) continue;
        const float d = dist[row];
        if (!(__builtin_fabsf(d) < __builtin_inff())) continue;
        const int64_t key = make_key(d, row);
        if (key > prev[rank]) offer_key(cur + rank, key);
    }
}

// cur -> member `j` of every rank and its previous pick; cur re-armed. An exhausted group hands on KEY_PAD, which nothing is greater than.
__global__ __launch_bounds__(256) void group_advance_kernel(int64_t* cur, int64_t* prev, int64_t* member_keys, int32_t limit, int32_t per_group, int32_t j) {
    const int32_t rank = (int32_t)(blockIdx.x * 256u + threadIdx.x);
    if (rank >= limit) return;
    const int64_t c = cur[rank];
    member_keys[(size_t)rank * per_group + j] = c;
    prev[rank] = c;
    cur[rank] = KEY_PAD;
}

__global__ __launch_bounds__(256) void group_ids_kernel(const int64_t* __restrict__ member_keys, uint32_t n, const uint64_t* __restrict__ row_ids,
                                                        uint32_t n_rows, uint64_t* __restrict__ member_ids) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int64_t k = member_keys[i];
    const uint32_t row = key_row(k);
    member_ids[i] = (k != KEY_PAD && row < n_rows) ? row_ids[row] : ID_PAD;
}

hipError_t launch_group_select(const GroupSelectArgs& a, hipStream_t st) {
    if (a.limit < 1 || a.limit > GROUP_MAX_LIMIT || a.per_group < 0 || a.per_group > GROUP_MAX_MEMBERS || a.n_slots == 0 || a.best == nullptr ||
        a.dist_col == nullptr || a.tl_scratch == nullptr || a.out == nullptr)
        return hipErrorInvalidValue;
    if (a.per_group > 0 && (a.rank_of_slot == nullptr || a.cur == nullptr)) return hipErrorInvalidValue;
    if (a.per_group > 1 && (a.dist == nullptr || a.n_rows == 0 || (a.slots == nullptr && a.n_slots < a.n_rows))) return hipErrorInvalidValue;
    const uint32_t L = (uint32_t)a.limit, P = (uint32_t)a.per_group;
    uint64_t* out_roots = reinterpret_cast<uint64_t*>(a.out);
    int64_t* out_dist = a.out + L;
    uint32_t* out_count = reinterpret_cast<uint32_t*>(a.out + 2ull * L);
    int64_t* member_keys = a.out + 2ull * L + 1ull;
    int64_t* member_ids = member_keys + (size_t)L * P;
    int64_t* cur = a.cur;
    int64_t* prev = a.cur != nullptr ? a.cur + L : nullptr;
    const uint32_t slot_blocks = row_grid(a.n_slots, 0u);

    hipLaunchKernelGGL(group_split_kernel, dim3(slot_blocks), dim3(256), 0, st, a.best, a.n_slots, a.dist_col);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    TimelineArgs t{};
    t.ts = a.dist_col; t.flags = nullptr; t.ids = a.slot_root; t.n_rows = a.n_slots;
    t.limit = a.limit; t.newest = 0;
    t.has_after = 0; t.after = 0; t.has_before = 1; t.before = INT64_MAX; t.deny_flags = 0u;   // an empty slot (INT64_MAX) is no candidate
    t.out_ids = out_roots; t.out_ts = out_dist; t.out_count = out_count;
    err = launch_timeline(t, timeline_grid(a.n_slots, a.limit), a.tl_scratch, st);
    if (err != hipSuccess || P == 0u) return err;

    err = fill_words(member_keys, (uint64_t)L * P, KEY_PAD, st);
    if (err == hipSuccess) err = fill_words(member_ids, (uint64_t)L * P, (int64_t)ID_PAD, st);
    if (err == hipSuccess) err = fill_words(cur, 2ull * L, KEY_PAD, st);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(group_mark_kernel, dim3(slot_blocks), dim3(256), 0, st, a.best, a.slot_root, a.n_slots, out_roots, out_dist, out_count,
                       a.limit, a.per_group, a.rank_of_slot, member_keys, prev);
    err = hipGetLastError();
    const uint32_t round_blocks = row_grid(a.n_rows, a.grid);
    for (int32_t j = 1; j < a.per_group && err == hipSuccess; ++j) {
        hipLaunchKernelGGL(group_round_kernel, dim3(round_blocks), dim3(256), 0, st, a.dist, a.slots, a.bitmap, a.n_rows, a.n_slots,
                           a.rank_of_slot, prev, a.limit, cur);
        hipLaunchKernelGGL(group_advance_kernel, dim3((L + 255u) / 256u), dim3(256), 0, st, cur, prev, member_keys, a.limit, a.per_group, j);
        err = hipGetLastError();
    }
    if (err == hipSuccess && a.row_ids != nullptr) {
        hipLaunchKernelGGL(group_ids_kernel, dim3((L * P + 255u) / 256u), dim3(256), 0, st, member_keys, L * P, a.row_ids, a.n_rows,
                           reinterpret_cast<uint64_t*>(member_ids));
        err = hipGetLastError();
    }
    return err;
}

}  // namespace wax
