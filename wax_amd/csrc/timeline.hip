// timeline.hip — device side of wax_hip_timeline (Wax.timeline, TimelineQuery.swift:38-53): the `limit` newest or
// oldest rows that pass a row predicate, straight from the attribute columns.
//
// The key of a row is the PAIR (t', id), compared lexicographically with t' signed and id unsigned: t' = ts for chronological order,
// ~ts for newest-first (~ reverses the order of int64 without the overflow -ts has at INT64_MIN), id = the row's frame id. Frame ids
// are unique in a store, so keys are distinct and the `limit` smallest are one well-defined set in one order.
//
//   timeline_select_kernel   256 threads; workgroups walk 256-row tiles grid-strided, in a permuted tile order (timeline_tile_stride:
//                            a store appended in time order, walked against the order asked for, would otherwise hand every row to
//                            the buffer). A lane reads its row's timestamp and flag word coalesced, applies attr_row_passes, and tests
//                            t' against the workgroup's current k-th pair; the frame id is loaded only where t' does not already
//                            decide against the row. Survivors are appended to an LDS pair buffer by ballot / mbcnt rank, one LDS add
//                            per wave. When a further tile would not fit — and once as soon as `limit` pairs are there — the buffer
//                            is sorted (bitonic, padded to a power of two), cut to `limit` and its last pair becomes the threshold.
//                            At the end: sort, and the list, ascending, to the partials (position-major).
//   timeline_merge_kernel    one workgroup, the same frame over the partial lists, 256 lists' entries of one position per tile, from
//                            the heads on; 256 lists whose tile leaves no survivor are done with. Writes ids (padded with
//                            UINT64_MAX), timestamps and the count.
//
// The buffer's capacity is a launch parameter (dynamic LDS): 512 / 2 048 / 8 192 pairs for limit <= 256 / 1 024 / 4 096, always at
// least limit + 256, so a tile fits behind every cut. The largest is 128 KB of the CU's 160 KB.
#include <cmath>

#include "kernels.h"
#include "topk.h"

namespace wax {

namespace {

constexpr int64_t T_PAD = INT64_MAX;

__device__ inline bool pair_less(int64_t ta, uint64_t ia, int64_t tb, uint64_t ib) { return ta < tb || (ta == tb && ia < ib); }

// The workgroup's selection frame. `n` (pairs in the buffer) is kept uniform in registers: every wave posts its tile count to
// wave_cnt[parity] and every thread adds the four after the tile's barrier (a wave is at most one tile ahead of the slowest reader,
// so two parities suffice); *fill is the allocation word the waves add to.
struct PairFrame {
    int64_t* t;
    uint64_t* id;
    uint32_t* fill;
    uint32_t* wave_cnt;     // [2][4]
    uint32_t cap, limit;
    uint32_t n;
    uint32_t parity;
    bool have_thr;
    int64_t thr_t;
    uint64_t thr_id;
};

__device__ inline void frame_init(PairFrame& f, unsigned char* lds, uint32_t cap, uint32_t limit) {
    f.t = reinterpret_cast<int64_t*>(lds);
    f.id = reinterpret_cast<uint64_t*>(lds + (size_t)cap * 8u);
    f.fill = reinterpret_cast<uint32_t*>(lds + (size_t)cap * 16u);
    f.wave_cnt = f.fill + 4;
    f.cap = cap; f.limit = limit; f.n = 0; f.parity = 0; f.have_thr = false; f.thr_t = T_PAD; f.thr_id = ID_PAD;
    if (threadIdx.x == 0) *f.fill = 0u;
    __syncthreads();
}

// Sort the n pairs ascending (every thread of the workgroup; entries [n, N) are padding), keep min(n, limit), tighten the threshold.
__device__ inline void frame_cut(PairFrame& f) {
    uint32_t N = 2;
    while (N < f.n) N <<= 1;                                     // N <= cap: cap is a power of two and n <= cap
    for (uint32_t i = f.n + threadIdx.x; i < N; i += 256u) { f.t[i] = T_PAD; f.id[i] = ID_PAD; }
    __syncthreads();
    for (uint32_t k = 2; k <= N; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t p = threadIdx.x; p < (N >> 1); p += 256u) {
                const uint32_t i = ((p & ~(j - 1u)) << 1) | (p & (j - 1u));   // the pair's lower index: bit j clear
                const uint32_t l = i | j;
                const int64_t ta = f.t[i], tb = f.t[l];
                const uint64_t ia = f.id[i], ib = f.id[l];
                const bool up = (i & k) == 0u;
                if (up ? pair_less(tb, ib, ta, ia) : pair_less(ta, ia, tb, ib)) {
                    f.t[i] = tb; f.id[i] = ib; f.t[l] = ta; f.id[l] = ia;
                }
            }
            __syncthreads();
        }
    }
    if (f.n > f.limit) f.n = f.limit;
    if (f.n == f.limit) { f.have_thr = true; f.thr_t = f.t[f.limit - 1u]; f.thr_id = f.id[f.limit - 1u]; }
    __syncthreads();                                             // (the threshold is read before the next tile's appends)
    if (threadIdx.x == 0) *f.fill = f.n;
    __syncthreads();
}

// One tile: this lane's entry (valid, t') of source index idx; load_id(idx) fetches its id only if the entry survives t'.
// Returns the tile's survivors (uniform). The buffer is cut when a further tile would not fit, and once as soon as it holds `limit`
// pairs: the first threshold then comes from a small sort, and what follows is mostly rejected on t' alone.
template <typename LoadId>
__device__ inline uint32_t frame_offer(PairFrame& f, bool valid, int64_t tp, uint64_t idx, LoadId load_id, bool* kept = nullptr) {
    if (f.n + 256u > f.cap || (!f.have_thr && f.n >= f.limit)) frame_cut(f);   // uniform: n and have_thr are
    bool keep = valid;
    uint64_t fid = 0;
    if (keep) {
        if (f.have_thr && tp > f.thr_t) keep = false;
        else {
            fid = load_id(idx);
            if (f.have_thr && tp == f.thr_t) keep = fid < f.thr_id;
        }
    }
    if (kept != nullptr) *kept = keep;
    const unsigned long long b = __ballot(keep);
    const uint32_t cnt = (uint32_t)__popcll(b);
    const uint32_t rank = (uint32_t)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
    const int lane = lane_id();
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t base = 0;
    if (lane == 0) {
        if (cnt != 0u) base = atomicAdd(f.fill, cnt);
        f.wave_cnt[f.parity * 4u + wave] = cnt;
    }
    base = (uint32_t)__shfl((int)base, 0);
    if (keep) { f.t[base + rank] = tp; f.id[base + rank] = fid; }   // base + rank < n + 256 <= cap
    __syncthreads();
    const uint32_t* wc = f.wave_cnt + f.parity * 4u;
    const uint32_t got = wc[0] + wc[1] + wc[2] + wc[3];
    f.n += got;
    f.parity ^= 1u;
    return got;
}

}  // namespace

__global__ __launch_bounds__(256) void timeline_select_kernel(TimelineArgs a, uint32_t cap) {
    extern __shared__ __align__(16) unsigned char tl_lds[];
    PairFrame f;
    frame_init(f, tl_lds, cap, (uint32_t)a.limit);
    const uint64_t n_tiles = (a.n_rows + 255ull) / 256ull;
    const uint64_t* ids = a.ids;
    auto load_id = [ids](uint64_t row) { return ids != nullptr ? ids[row] : row; };
    auto load_row = [&a, n_tiles](uint64_t step, uint64_t* row, int64_t* ts, uint32_t* fl) {
        *row = UINT64_MAX; *ts = 0; *fl = 0u;
        if (step >= n_tiles) return;
        const uint64_t tile = (step * a.tile_stride) % n_tiles;   // a permutation of the tiles: tile_stride is coprime to n_tiles
        const uint64_t r = tile * 256ull + threadIdx.x;
        if (r >= a.n_rows) return;
        *row = r;
        *ts = a.ts != nullptr ? a.ts[r] : 0;
        *fl = a.flags != nullptr ? a.flags[r] : 0u;
    };
    uint64_t row, row_next;
    int64_t ts, ts_next;
    uint32_t fl, fl_next;
    load_row(blockIdx.x, &row, &ts, &fl);
    for (uint64_t step = blockIdx.x; step < n_tiles; step += gridDim.x) {
        load_row(step + gridDim.x, &row_next, &ts_next, &fl_next);   // the next tile's loads are in flight while this one is offered
        const bool valid = row != UINT64_MAX && attr_row_passes(a.has_after, a.after, a.has_before, a.before, a.deny_flags, ts, fl);
        frame_offer(f, valid, a.newest != 0 ? ~ts : ts, row, load_id);
        row = row_next; ts = ts_next; fl = fl_next;
    }
    frame_cut(f);
    // position-major: entry i of every list side by side, so the merge reads the lists' heads coalesced
    for (uint32_t i = threadIdx.x; i < f.n; i += 256u) {
        const uint64_t slot = (uint64_t)i * gridDim.x + blockIdx.x;
        a.part_t[slot] = f.t[i];
        a.part_id[slot] = f.id[i];
    }
    if (threadIdx.x == 0) a.part_cnt[blockIdx.x] = f.n;
}

__global__ __launch_bounds__(256) void timeline_merge_kernel(TimelineArgs a, uint32_t n_lists, uint32_t cap) {
    extern __shared__ __align__(16) unsigned char tl_lds[];
    PairFrame f;
    frame_init(f, tl_lds, cap, (uint32_t)a.limit);
    const uint64_t* part_id = a.part_id;
    auto load_id = [part_id](uint64_t p) { return part_id[p]; };
    // A tile is position `pos` of the 256 lists of one group. Every list ascends, so a group whose tile leaves no survivor — all
    // beyond the threshold, which only tightens, or beyond their lists' ends — has none at any later position either: it is dead.
    constexpr uint32_t kGroups = TIMELINE_MAX_GRID / 256u;
    const uint32_t groups = (n_lists + 255u) / 256u;             // <= kGroups: launch_timeline checks the grid
    uint32_t cnt[kGroups];
    for (uint32_t g = 0; g < kGroups; ++g) {
        const uint32_t list = g * 256u + threadIdx.x;
        cnt[g] = list < n_lists ? a.part_cnt[list] : 0u;
    }
    // A group with only a few lists left is finished list by list instead, 256 POSITIONS of one list per tile (strided reads, but a
    // list that holds much of the answer — the last rows of a store appended in time order belong to a handful of workgroups — then
    // costs limit / 256 tiles, not `limit` of them): a list is walked while whole tiles of it survive.
    constexpr uint32_t kColumnLists = 16;
    unsigned long long* col_mask = reinterpret_cast<unsigned long long*>(tl_lds + (size_t)cap * 16u + 64u);   // [4], one per wave
    uint32_t live = groups;
    uint32_t dead = 0;
    for (uint32_t pos = 0; pos < (uint32_t)a.limit && live != 0u; ++pos) {
        for (uint32_t g = 0; g < kGroups; ++g) {
            if (g >= groups || ((dead >> g) & 1u) != 0u) continue;   // uniform
            const bool valid = pos < cnt[g];
            const uint64_t p = (uint64_t)pos * n_lists + g * 256u + threadIdx.x;
            const int64_t tp = valid ? a.part_t[p] : T_PAD;
            bool kept = false;
            const uint32_t got = frame_offer(f, valid, tp, p, load_id, &kept);
            if (got > kColumnLists) continue;
            dead |= 1u << g; --live;
            if (got == 0u || pos + 1u >= (uint32_t)a.limit) continue;
            const unsigned long long b = __ballot(kept);
            if (lane_id() == 0) col_mask[threadIdx.x >> 6] = b;
            __syncthreads();
            unsigned long long m[4] = {col_mask[0], col_mask[1], col_mask[2], col_mask[3]};
            for (uint32_t w = 0; w < 4u; ++w) {
                while (m[w] != 0ull) {
                    const uint32_t list = g * 256u + w * 64u + (uint32_t)__builtin_ctzll(m[w]);
                    m[w] &= m[w] - 1ull;
                    const uint32_t len = a.part_cnt[list];
                    for (uint32_t q0 = pos + 1u; q0 < len; q0 += 256u) {
                        const uint32_t q = q0 + threadIdx.x;
                        const uint64_t pq = (uint64_t)q * n_lists + list;
                        const int64_t tq = q < len ? a.part_t[pq] : T_PAD;
                        const uint32_t want = len - q0 < 256u ? len - q0 : 256u;
                        if (frame_offer(f, q < len, tq, pq, load_id) < want) break;   // ascending: nothing behind a rejected entry survives
                    }
                }
            }
        }
    }
    frame_cut(f);
    for (uint32_t i = threadIdx.x; i < (uint32_t)a.limit; i += 256u) {
        a.out_ids[i] = i < f.n ? f.id[i] : ID_PAD;
        if (a.out_ts != nullptr) a.out_ts[i] = i < f.n ? (a.newest != 0 ? ~f.t[i] : f.t[i]) : 0;
    }
    if (threadIdx.x == 0) *a.out_count = f.n;
}

uint32_t timeline_buffer_pairs(int32_t limit) { return limit <= 256 ? 512u : (limit <= 1024 ? 2048u : 8192u); }

// Workgroups of the scan: one per tile up to four per CU for the two smaller buffers (a workgroup's walk is a chain of tile steps,
// each a load latency and a barrier long: the more workgroups, the shorter the chain), one per CU for the largest (128 KB of LDS
// each). The merge walks the lists from their heads and drops 256 lists at a time, so its cost does not grow with grid x limit.
uint32_t timeline_grid(uint64_t n_rows, int32_t limit) {
    const uint64_t tiles = (n_rows + 255ull) / 256ull;
    uint64_t g = limit <= 1024 ? (uint64_t)TIMELINE_MAX_GRID : 256ull;
    if (g > tiles) g = tiles;
    return (uint32_t)(g < 1ull ? 1ull : g);
}

// The walk's multiplier: step s of the walk is tile (s * stride) mod n_tiles, a permutation because stride is coprime to n_tiles.
// A store appended in time order then looks like a shuffled one to every workgroup, whichever order is asked for: after its first
// cut the threshold rejects most rows on t' alone, where a walk against the order would hand every row to the buffer. A workgroup
// takes steps b, b + grid, b + 2 grid, ...: its own tiles advance by grid * stride mod n_tiles, so among the coprime candidates near
// n_tiles / golden ratio the one is taken whose per-workgroup advance is closest to n_tiles / golden ratio as well — neither the
// workgroups' first tiles nor one workgroup's successive tiles then run along the store.
static uint64_t timeline_tile_stride(uint64_t n_tiles, uint32_t grid) {
    if (n_tiles < 3ull) return 1ull;
    constexpr double kGolden = 0.6180339887498949;
    auto gcd = [](uint64_t x, uint64_t y) { while (y != 0ull) { const uint64_t r = x % y; x = y; y = r; } return x; };
    uint64_t best = 0;
    double best_err = 2.0;
    uint64_t m = (uint64_t)((double)n_tiles * kGolden) | 1ull;
    for (int tried = 0; tried < 128; m += 2ull) {
        if (gcd(m, n_tiles) != 1ull) continue;                   // (odd numbers coprime to n_tiles are never further than a few steps apart)
        ++tried;
        const double adv = (double)((m % n_tiles) * (uint64_t)grid % n_tiles) / (double)n_tiles;
        const double err = std::fabs(adv - kGolden) < std::fabs(adv - (1.0 - kGolden)) ? std::fabs(adv - kGolden) : std::fabs(adv - (1.0 - kGolden));
        if (err < best_err) { best_err = err; best = m; }
    }
    return best % n_tiles;
}

uint64_t timeline_scratch_words(uint32_t grid, int32_t limit) {
    return 2ull * (uint64_t)grid * (uint64_t)limit + ((uint64_t)grid + 1ull) / 2ull;
}

hipError_t launch_timeline(const TimelineArgs& args, uint32_t grid, int64_t* d_scratch, hipStream_t st) {
    if (args.limit < 1 || args.limit > TIMELINE_MAX_LIMIT || grid < 1u || grid > TIMELINE_MAX_GRID || d_scratch == nullptr ||
        args.out_ids == nullptr || args.out_count == nullptr)
        return hipErrorInvalidValue;
    TimelineArgs a = args;
    const uint64_t pairs = (uint64_t)grid * (uint64_t)a.limit;
    a.part_t = d_scratch;
    a.part_id = reinterpret_cast<uint64_t*>(d_scratch + pairs);
    a.part_cnt = reinterpret_cast<uint32_t*>(d_scratch + 2ull * pairs);
    a.tile_stride = timeline_tile_stride((a.n_rows + 255ull) / 256ull, grid);
    const uint32_t cap = timeline_buffer_pairs(a.limit);
    const uint32_t smem = cap * 16u + 96u;
    static std::atomic<uint64_t> done_select{0}, done_merge{0};
    const size_t smem_max = (size_t)timeline_buffer_pairs(TIMELINE_MAX_LIMIT) * 16u + 96u;
    hipError_t err = ensure_dynamic_lds(reinterpret_cast<const void*>(&timeline_select_kernel), smem_max, done_select);
    if (err == hipSuccess) err = ensure_dynamic_lds(reinterpret_cast<const void*>(&timeline_merge_kernel), smem_max, done_merge);
    if (err != hipSuccess) return err;
    launch_kernel(timeline_select_kernel, dim3(grid), dim3(256), smem, st, a, cap);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(timeline_merge_kernel, dim3(1), dim3(256), smem, st, a, grid, cap);
    return hipGetLastError();
}

}  // namespace wax
