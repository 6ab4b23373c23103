// topk.h — wavefront-private streaming top-k and workgroup rank-merge (device only).
//
// Replaces the reference's multi-pass GPU selection (TopKReduction.metal:103-167:
// per-256-chunk lane-0 heap or bitonic sort, iterated with one launch and one
// fresh buffer per pass, MetalVectorEngine.swift:511-575) with a design that
// fits CDNA4: every 64-lane wave keeps a private candidate list in LDS behind a
// running threshold `tau` (the wave's current k-th smallest key), so that after
// warm-up almost every row is rejected with one 64-bit compare and the
// selection costs ~0 next to the HBM stream. Keys are unique 64-bit integers
// (ordered distance : row), so order is total and deterministic.
#pragma once
#include "common.h"

namespace wax {

__device__ inline int lane_id() { return (int)(threadIdx.x & 63); }

// Compiler-level ordering point for LDS traffic inside ONE wave. A wave's DS
// instructions execute in order, so no hardware wait is needed between a
// ds_write and a later ds_read of another lane's data; this only stops hipcc
// from reordering across the point.
__device__ inline void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

typedef __attribute__((address_space(3))) int64_t lds_i64;

struct PruneOut {
    int cnt;
    int64_t tau;
};

// Rank-sort the `cnt` live candidates of one wave's list, keep the k smallest in
// buf[0..min(cnt,k)) ascending, return the new count and threshold. O(cnt*CAP/64) compares per
// lane, no inter-lane shuffles. Deliberately NOT inlined: it is cold code (a wave prunes a handful
// of times per launch) and every inlined copy is ~3 KB of instructions that a single-workgroup
// kernel pays for in instruction-cache misses (merge_keys_kernel: 5 500 lines of ISA, 20 us).
// UNIQUE: the caller guarantees that no key occurs twice (keys carry the global row in their low half, and every
// internal producer offers a row once), so a rank is just the number of smaller keys: one 64-bit compare per pair
// instead of three compares. Lists of foreign keys (gathered shard hits) use UNIQUE = false, which orders duplicates
// by slot index. Slices of 64 slots beyond the live count are skipped (wave-uniform).
template <int CAP, bool UNIQUE>
__device__ __attribute__((noinline)) PruneOut wave_prune(lds_i64* buf, int cnt, int k) {
    constexpr int E = CAP / 64;
    wave_lds_fence();
    const int lane = lane_id();
    int64_t mine[E];
    int rank[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int idx = lane + 64 * e;
        mine[e] = (idx < cnt) ? buf[idx] : KEY_PAD;
        rank[e] = 0;
    }
    const int live = __builtin_amdgcn_readfirstlane(cnt);
    // 4 broadcast keys per trip (two ds_read_b128): the loop is LDS-latency-bound otherwise.
    int j = 0;
    for (; j + 4 <= live; j += 4) {
        int64_t o[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) o[u] = buf[j + u];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (64 * e < live) {
                const int idx = lane + 64 * e;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (UNIQUE) rank[e] += (o[u] < mine[e]) ? 1 : 0;
                    else rank[e] += (o[u] < mine[e] || (o[u] == mine[e] && (j + u) < idx)) ? 1 : 0;
                }
            }
        }
    }
    for (; j < live; ++j) {
        const int64_t o = buf[j];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int idx = lane + 64 * e;
            if (UNIQUE) rank[e] += (o < mine[e]) ? 1 : 0;
            else rank[e] += (o < mine[e] || (o == mine[e] && j < idx)) ? 1 : 0;
        }
    }
    wave_lds_fence();
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int idx = lane + 64 * e;
        if (idx < cnt && rank[e] < k) buf[rank[e]] = mine[e];
    }
    wave_lds_fence();
    PruneOut r;
    r.cnt = cnt < k ? cnt : k;
    r.tau = (r.cnt >= k) ? buf[k - 1] : KEY_PAD;
    return r;
}

// wave_prune<CAP, true> with k = 64 for a list that an earlier prune left full: buf[0 .. 64) are the 64 smallest keys so far,
// ascending, and buf[64 .. cnt) the m = cnt - 64 >= 1 keys pushed since. Lane l owns old key l and new key l. An old key's rank is
// its index plus the new keys below it; a new key's rank is the old keys below it — a binary search in the sorted prefix, one step
// per trip of the loop — plus the new keys below it. m broadcast keys and 2 m compares per lane where the general prune has
// 64 + m and 2 (64 + m), and the result is the same: the 64 smallest in buf[0 .. 64) ascending, tau = buf[63].
template <int CAP>
__device__ __attribute__((noinline)) PruneOut wave_prune_sorted(lds_i64* buf, int cnt) {
    constexpr int K = 64, STEPS = 7;                        // a search over 64 entries ends within 7 steps
    static_assert(CAP - K <= 64 && (CAP - K) % 4 == 0, "one new key per lane, four per trip");
    wave_lds_fence();
    const int lane = lane_id();
    const int m = __builtin_amdgcn_readfirstlane(cnt) - K;
    const int64_t old = buf[lane];
    const int64_t nw = (lane < m) ? buf[K + lane] : KEY_PAD;
    int rank_old = lane, below = 0, lo = 0, hi = K;
    auto search_step = [&]() {
        const bool open = lo < hi;
        const int mid = open ? (lo + hi) >> 1 : 0;
        const bool before = buf[mid] < nw;
        lo = (open && before) ? mid + 1 : lo;
        hi = (open && !before) ? mid : hi;
    };
    int steps = 0;
    for (int j = 0; j < m; j += 4) {
        int64_t o[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) o[u] = buf[K + j + u];
        if (steps < STEPS) { search_step(); ++steps; }      // (wave-uniform)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t key = (j + u < m) ? o[u] : KEY_PAD;     // a slot past the live ones holds an old key
            rank_old += (key < old) ? 1 : 0;
            below += (key < nw) ? 1 : 0;
        }
    }
    for (; steps < STEPS; ++steps) search_step();
    const int rank_new = lo + below;
    wave_lds_fence();
    if (rank_old < K) buf[rank_old] = old;
    if (lane < m && rank_new < K) buf[rank_new] = nw;
    wave_lds_fence();
    PruneOut r;
    r.cnt = K;
    r.tau = buf[K - 1];
    return r;
}

// Streaming k-smallest over int64 keys, private to one wave.
//   CAP  : LDS slots (power of two, >= k + 64 so that one push of up to 64
//          candidates always fits after a prune)
template <int CAP, bool UNIQUE = true>
struct WaveTopK {
    static_assert(CAP % 64 == 0, "CAP must be a multiple of the wave size");

    int64_t* buf;  // CAP slots in LDS, this wave only
    int cnt;       // wave-uniform number of live candidates in buf[0..cnt)
    int k;         // wave-uniform
    int64_t tau;   // wave-uniform: only keys < tau can still enter the top-k

    __device__ inline void init(int64_t* lds, int k_) {
        buf = lds;
        cnt = 0;
        k = k_;
        tau = KEY_PAD;
    }

    // Every lane of the wave must call push() together (valid=false for idle lanes). The caller
    // guarantees room: cnt + (number of valid lanes) <= CAP, by calling make_room() first.
    __device__ inline void push(int64_t key, bool valid) {
        const bool pass = valid && (key < tau);
        const unsigned long long mask = __ballot(pass);
        if (mask == 0ull) return;  // wave-uniform
        const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                                     __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        if (pass) buf[cnt + before] = key;
        cnt += __popcll(mask);
    }

    // Ensure the next `incoming` (<= 64, or <= CAP - k) candidates fit; prunes at most once.
    __device__ inline void make_room(int incoming) {
        if (cnt > CAP - incoming) prune();
    }

    // push() for kernels that offer up to 64 candidates at once: prunes only when the candidates
    // that actually pass the threshold do not fit (a fixed make_room(64) would prune after every
    // insertion once k >= CAP - 64).
    __device__ inline void push_wide(int64_t key, bool valid) {
        bool pass = valid && (key < tau);
        unsigned long long mask = __ballot(pass);
        if (mask == 0ull) return;
        if (cnt + __popcll(mask) > CAP) {
            prune();  // cnt <= k <= CAP - 64 afterwards, tau tightened: re-test
            pass = valid && (key < tau);
            mask = __ballot(pass);
            if (mask == 0ull) return;
        }
        const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                                     __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        if (pass) buf[cnt + before] = key;
        cnt += __popcll(mask);
    }

    __device__ inline void prune() {
        const PruneOut r = wave_prune<CAP, UNIQUE>((lds_i64*)buf, cnt, k);
        cnt = r.cnt;
        tau = r.tau;
    }

    __device__ inline void finalize() { prune(); }
};

// Merge the sorted per-wave lists of a workgroup by ranking: an entry's final
// position is its own index plus, for every other wave, the number of that
// wave's entries ordered before it (binary search). One pass, one barrier.
//   lists  : LDS, wave w's sorted list at lists + w*stride, length counts[w] (<= k)
//   out    : k slots (global or LDS); slots past the merged total get KEY_PAD
// Must be called by all threads of the block; ends with all writes issued (no trailing barrier).
typedef __attribute__((address_space(3))) int lds_i32;

// Not inlined and not unrolled for the same instruction-footprint reason as wave_prune.
__device__ __attribute__((noinline)) void block_rank_merge_impl(const lds_i64* lists, int nwaves, int stride,
                                                                const lds_i32* counts, int k, int64_t* out) {
    const int tid = (int)threadIdx.x;
    const int nthreads = (int)blockDim.x;
    int total = 0;
    for (int w = 0; w < nwaves; ++w) total += counts[w];
    const int total_k = total < k ? total : k;
    for (int t = tid; t < nwaves * k; t += nthreads) {
        const int w = t / k, i = t - w * k;
        if (i >= counts[w]) continue;
        const int64_t key = lists[w * stride + i];
        int rank = i;
        for (int o = 0; o < nwaves; ++o) {
            if (o == w) continue;
            // number of entries in list o that precede `key` (ties: lower wave index first)
            int lo = 0, hi = counts[o];
            const lds_i64* lst = lists + o * stride;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const int64_t v = lst[mid];
                const bool before = (o < w) ? (v <= key) : (v < key);
                if (before) lo = mid + 1; else hi = mid;
            }
            rank += lo;
        }
        if (rank < k) out[rank] = key;
    }
    for (int t = total_k + tid; t < k; t += nthreads) out[t] = KEY_PAD;
}

template <int NWAVES>
__device__ inline void block_rank_merge(const int64_t* lists, int stride, const int* counts, int k,
                                        int64_t* out) {
    block_rank_merge_impl((const lds_i64*)lists, NWAVES, stride, (const lds_i32*)counts, k, out);
}

// ---- DPP cross-lane adds (no LDS traffic) ---------------------------------
// v + (v moved by a DPP pattern); lanes in rows excluded by ROW_MASK add +0.0.
template <int CTRL, int ROW_MASK>
__device__ inline float dpp_add(float v) {
    const int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, false);
    return v + __int_as_float(moved);
}

// Sum over each aligned group of GROUP lanes. The total is valid in the LAST
// lane of each group (for GROUP <= 16 in every lane of the group).
template <int GROUP>
__device__ inline float group_sum(float v) {
    static_assert(GROUP == 4 || GROUP == 8 || GROUP == 16 || GROUP == 32 || GROUP == 64, "GROUP");
    v = dpp_add<0xB1, 0xF>(v);                         // quad_perm [1,0,3,2]
    v = dpp_add<0x4E, 0xF>(v);                         // quad_perm [2,3,0,1]
    if (GROUP >= 8) v = dpp_add<0x141, 0xF>(v);        // row_half_mirror
    if (GROUP >= 16) v = dpp_add<0x140, 0xF>(v);       // row_mirror
    if (GROUP >= 32) v = dpp_add<0x142, 0xA>(v);       // row_bcast15 into rows 1,3
    if (GROUP >= 64) v = dpp_add<0x143, 0xC>(v);       // row_bcast31 into rows 2,3
    return v;
}

// ---- last arriver of a fused scan (kernels.hip) and the mirror scan's finish (mirror_scan.hip), small k: a k-way merge of the per-workgroup lists instead of streaming them through the wave lists -----------
// The lists are sorted, so the global best key is the smallest of the lists' HEADS. Thread t owns lists t, t + 256, ... (LISTS of
// them: 1 for the small grids, 2 up to SCAN_KWAY_MERGE_GRID) and keeps the next four keys of each in registers; k rounds of
// {workgroup-wide minimum of the heads by DPP + one LDS exchange, the owner of the minimum emits it and advances that list} produce
// the k best in order. A round is a few hundred cycles and one barrier whatever the number of lists; the wave-list path (157 lists,
// k = 10: eight 64-key pushes with two rank-sort prunes per wave, a final prune, a rank merge) took ~10 of the ~20 us a 10K-row
// query spends in this kernel, and grows with the grid. Keys are unique (distinct rows) except KEY_PAD, which nobody "wins".
template <int CTRL>
__device__ inline int64_t dpp_min_i64(int64_t v) {
    const int lo = __builtin_amdgcn_update_dpp((int)(uint32_t)v, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(v >> 32), (int)(v >> 32), CTRL, 0xF, 0xF, false);
    const int64_t o = (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
    return o < v ? o : v;
}
__device__ inline int64_t readlane_i64(int64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
template <int LISTS>
__device__ __attribute__((noinline)) void kway_merge(const int64_t* partials, int nlists, int k, int64_t* fin, int64_t* xch) {
    const int t = (int)threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    int64_t h[LISTS][4];
    int taken[LISTS];
#pragma unroll
    for (int j = 0; j < LISTS; ++j) {
        const int64_t* lst = partials + (size_t)(t + j * SCAN_THREADS) * k;
        taken[j] = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            h[j][i] = (t + j * SCAN_THREADS < nlists && i < k) ? __hip_atomic_load(lst + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : KEY_PAD;
    }
    for (int r = 0; r < k; ++r) {
        int64_t head[LISTS];
#pragma unroll
        for (int j = 0; j < LISTS; ++j) {
            const int sel = taken[j] & 3;
            head[j] = sel == 0 ? h[j][0] : sel == 1 ? h[j][1] : sel == 2 ? h[j][2] : h[j][3];
        }
        int64_t mine = head[0];
#pragma unroll
        for (int j = 1; j < LISTS; ++j) mine = head[j] < mine ? head[j] : mine;
        int64_t v = mine;
        v = dpp_min_i64<0xB1>(v);       // quad_perm [1,0,3,2]
        v = dpp_min_i64<0x4E>(v);       // quad_perm [2,3,0,1]
        v = dpp_min_i64<0x141>(v);      // row_half_mirror
        v = dpp_min_i64<0x140>(v);      // row_mirror: every lane holds its row's (16 lanes) minimum
        int64_t w = readlane_i64(v, 0);
        const int64_t w1 = readlane_i64(v, 16), w2 = readlane_i64(v, 32), w3 = readlane_i64(v, 48);
        w = w1 < w ? w1 : w; w = w2 < w ? w2 : w; w = w3 < w ? w3 : w;
        int64_t* slot = xch + (r & 1) * SCAN_WAVES;            // two sets of slots: one barrier per round
        if (lane == 0) slot[wave] = w;
        __syncthreads();
        int64_t best = slot[0];
#pragma unroll
        for (int i = 1; i < SCAN_WAVES; ++i) best = slot[i] < best ? slot[i] : best;
        if (best == KEY_PAD) {                                  // every list is exhausted: pad the rest
            if (t == 0) fin[r] = KEY_PAD;
            continue;
        }
        if (mine == best) {
            fin[r] = best;
#pragma unroll
            for (int j = 0; j < LISTS; ++j) {
                if (head[j] != best) continue;
                ++taken[j];
                if ((taken[j] & 3) == 0) {                       // the next four keys of this list (a run of neighbours in one workgroup's rows)
                    const int64_t* lst = partials + (size_t)(t + j * SCAN_THREADS) * k + taken[j];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        h[j][i] = (taken[j] + i < k) ? __hip_atomic_load(lst + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : KEY_PAD;
                }
            }
        }
    }
    __syncthreads();
}

// ---- the mirror finish (mirror_finish.h), k = MIRROR_KP = 64 behind ~500 lists: kway_merge's answer without its k barrier rounds ----
// (select_short_kernel's scheme, kernels.hip, at the finish's size.) The lists are sorted and their keys distinct rows, so any U with at
// least k keys <= U bounds the k-th key, and the keys <= U are a prefix of every list:
//   (1) U: thread (wave w, lane l) owns lists 4 l + w (+ SCAN_THREADS), so every wave holds a quarter of the lists whatever their
//       number. A lane's value is the distance word of its smallest head; the wave ranks its 64 values in registers (readlane, no
//       LDS) and takes the (k / SCAN_WAVES)-th; U is the largest of the four with every row under it. k / SCAN_WAVES lanes of each wave
//       have a head <= U: k distinct keys. (Looser than the k-th smallest head of all, by about a quarter more keys on a random store.)
//   (2) every list's prefix <= U into `buf` (GATHER_CAP keys of LDS) through one LDS counter (by estimate ~85 keys at ~500 lists of a random store);
//   (3) rank sort of the gathered keys: the first k into fin[0..k), KEY_PAD behind them when the lists hold fewer.
// Returns false, with fin untouched, when more than GATHER_CAP keys are <= U (the best rows in a few workgroups' lists, equal
// distances, fewer than k live heads above two lists): the caller runs kway_merge, whose answer this is in every other case.
// Ends with a barrier on either way out, so `ctl` (1 + SCAN_WAVES ints of LDS) and `buf` may be reused at once by the caller.
constexpr int GATHER_CAP = 128;
template <int LISTS>
__device__ __attribute__((noinline)) bool gather_select(const int64_t* __restrict__ partials, int nlists, int k, int64_t* fin, int64_t* buf, int* ctl) {
    const int t = (int)threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    int64_t h[LISTS][4];
    int x = INT32_MAX;
#pragma unroll
    for (int j = 0; j < LISTS; ++j) {
        const int list = lane * SCAN_WAVES + wave + j * SCAN_THREADS;
        const int64_t* lst = partials + (size_t)list * k;
#pragma unroll
        for (int i = 0; i < 4; ++i) h[j][i] = (list < nlists && i < k) ? lst[i] : KEY_PAD;
        const int hi = (int)(h[j][0] >> 32);
        x = hi < x ? hi : x;
    }
    // (1)
    int rank = 0;
#pragma unroll
    for (int l = 0; l < 64; ++l) {
        const int o = __builtin_amdgcn_readlane(x, l);
        rank += (o < x || (o == x && l < lane)) ? 1 : 0;
    }
    const int quota = k / SCAN_WAVES;
    if (rank == quota - 1) ctl[1 + wave] = x;                      // ranks are a permutation of 0 .. 63: one lane
    if (t == 0) ctl[0] = 0;
    __syncthreads();
    int u32 = ctl[1];
#pragma unroll
    for (int w = 1; w < SCAN_WAVES; ++w) u32 = ctl[1 + w] > u32 ? ctl[1 + w] : u32;
    const int64_t bound = (int64_t)(((uint64_t)(uint32_t)u32 << 32) | 0xffffffffull);
    // (2)
#pragma unroll
    for (int j = 0; j < LISTS; ++j) {
        const int64_t* lst = partials + (size_t)(lane * SCAN_WAVES + wave + j * SCAN_THREADS) * k;
        for (int i = 0; i < k;) {
            const int sel = i & 3;
            const int64_t key = sel == 0 ? h[j][0] : sel == 1 ? h[j][1] : sel == 2 ? h[j][2] : h[j][3];
            if (key == KEY_PAD || key > bound) break;
            const int pos = atomicAdd(&ctl[0], 1);
            if (pos >= GATHER_CAP) break;                          // overflow: the count alone is read below
            buf[pos] = key;
            ++i;
            if ((i & 3) == 0 && i < k) {                           // (h[j][0] != KEY_PAD: the list exists)
#pragma unroll
                for (int n = 0; n < 4; ++n) h[j][n] = (i + n < k) ? lst[i + n] : KEY_PAD;
            }
        }
    }
    __syncthreads();
    const int c = ctl[0];
    if (c > GATHER_CAP) {                                          // workgroup-uniform
        // `ctl` may be the k-way merge's exchange slots (mirror_finish: xch), which its first round writes before its first barrier:
        // every thread has read the count before any thread leaves
        __syncthreads();
        return false;
    }
    // (3)
    if (t < GATHER_CAP) {
        const int64_t key = t < c ? buf[t] : KEY_PAD;
        int r = 0;
        int j = 0;
        for (; j + 4 <= c; j += 4) {
#pragma unroll
            for (int n = 0; n < 4; ++n) r += (buf[j + n] < key) ? 1 : 0;
        }
        for (; j < c; ++j) r += (buf[j] < key) ? 1 : 0;
        if (t < c && r < k) fin[r] = key;
        if (t >= c && t < k) fin[t] = KEY_PAD;
    }
    __syncthreads();
    return true;
}

}  // namespace wax
