// predicate.hip — device side of wax_hip_search_predicate (passesFrameFilter, UnifiedSearch.swift:1241-1258):
// per-row attributes -> row bitmap, and the exact f32 scan that offers only the rows of that bitmap.
//
//   attr_mask_kernel     one lane per row: reads the timestamp and flag columns coalesced, evaluates the predicate, ballots, and
//                        writes the row bitmap filter.hip's allow-list path already has (with an allow-list: ANDs into the bitmap
//                        the probe kernel marked). Counts the passing rows and the scan chunks that hold one into two device words,
//                        and the live chunks of a second size (the mirror form's) into a third.
//   attr_mask_pooled_kernel  the same reads, test, ballot and word writes for MANY (store, predicate) records in one launch
//                        (wax_hip_search_many_predicate): one 256-row tile of one record per workgroup, no counters, no atomics.
//   attr_rows_count / scan / emit_kernel   the columns straight to compact ascending row lists with device-side counts, for MANY
//                        predicates in three plain launches (wax_hip_search_batch_predicate: the entries without an allow-list):
//                        work items of 4 096 rows, the same reads and test, ranks from ballots; no bitmap, no atomics.
//   scan_masked_kernel   scan_body's structure (kernels.hip): the same (dims -> GROUP) table, the same loads, accumulate / finish_row
//                        of row_math.h — a passing row's distance has the scan's bits. A wave reads its chunk's bits before the
//                        loads; a chunk without a passing row costs no load at all (the test is wave-uniform); otherwise a key is
//                        pushed only for a row whose bit is set. The per-workgroup lists go through the second-launch merge
//                        (merge_keys_kernel / select_short_kernel): no in-kernel last arriver, no completion word.
#include "kernels.h"
#include "row_math.h"
#include "topk.h"

namespace wax {

// The counters take ONE set of device atomics per workgroup: a workgroup walks 256-row tiles grid-strided, keeps its counts in
// registers, and the grid is capped at kMaskGrid. The first build had every wave add for itself (15 600 waves at 1M rows, all on
// the same two words). What is measured of that build (profiles/r13/c_routes_first_build.json): its gather route took 0.32 ms
// at 1/64 passing where the allow-list form — the same launches from the bitmap on — took 0.11. That the same-address atomics are
// the 0.2 ms in between is an inference from that table, not a kernel trace; this form is the remedy that inference calls for.
constexpr uint32_t kMaskGrid = 1024;

// (the per-row test itself, attr_row_passes, is in kernels.h: filter.hip's list sort applies it too)

__global__ __launch_bounds__(256) void attr_mask_kernel(AttrMaskArgs a) {
    __shared__ uint32_t wave_counts[4][3];
    const uint32_t n_words = (a.n_rows + 31u) / 32u;
    const uint32_t n_tiles = (a.n_rows + 255u) / 256u;
    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    // bit i * c of firsts(c): the first row of every aligned run of c rows among the wave's 64 (0: chunks of that size are not counted)
    auto firsts_of = [](uint32_t c) { return c >= 64u ? 1ull : (c != 0u ? ~0ull / ((1ull << c) - 1ull) : 0ull); };
    const unsigned long long firsts = firsts_of(a.chunk_rows), firsts2 = firsts_of(a.chunk_rows2);
    uint32_t n_pass = 0, n_chunks = 0, n_chunks2 = 0;           // wave-uniform
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t row = tile * 256u + threadIdx.x;
        bool pass = row < a.n_rows;
        if (pass) {
            const int64_t ts = a.ts != nullptr ? a.ts[row] : 0;
            const uint32_t fl = a.flags != nullptr ? a.flags[row] : 0u;
            pass = attr_row_passes(a.has_after, a.after, a.has_before, a.before, a.deny_flags, ts, fl);
            if (a.and_bitmap != 0) pass = pass && ((a.bitmap[row >> 5] >> (row & 31u)) & 1u) != 0u;   // (read by the wave that rewrites the word below)
        }
        const unsigned long long b = __ballot(pass);
        const uint32_t w0 = (row - (uint32_t)lane) >> 5;        // the wave's 64 rows are words w0, w0 + 1
        if (lane == 0 && w0 < n_words) a.bitmap[w0] = (uint32_t)b;
        if (lane == 32 && w0 + 1u < n_words) a.bitmap[w0 + 1u] = (uint32_t)(b >> 32);
        n_pass += (uint32_t)__popcll(b);
        // chunks are aligned runs of chunk_rows rows (a power of two <= 64): bit i of x = "a row of i .. i + chunk_rows - 1 passes"
        unsigned long long x = b;
        for (uint32_t s = 1; s < a.chunk_rows; s <<= 1) x |= x >> s;
        n_chunks += (uint32_t)__popcll(x & firsts);
        unsigned long long x2 = b;                              // the same for the second chunk size (the mirror form's: filter_host.inc)
        for (uint32_t s = 1; s < a.chunk_rows2; s <<= 1) x2 |= x2 >> s;
        n_chunks2 += (uint32_t)__popcll(x2 & firsts2);
    }
    if (lane == 0) { wave_counts[wave][0] = n_pass; wave_counts[wave][1] = n_chunks; wave_counts[wave][2] = n_chunks2; }
    __syncthreads();
    if (threadIdx.x < 3u) {
        const uint32_t v = wave_counts[0][threadIdx.x] + wave_counts[1][threadIdx.x] + wave_counts[2][threadIdx.x] + wave_counts[3][threadIdx.x];
        if (v != 0u) atomicAdd(&a.counts[threadIdx.x], v);
    }
}

hipError_t launch_attr_mask(const AttrMaskArgs& a, hipStream_t st) {
    if (a.n_rows == 0 || a.bitmap == nullptr || a.counts == nullptr) return hipErrorInvalidValue;
    if (a.chunk_rows > 64u || (a.chunk_rows & (a.chunk_rows - 1u)) != 0u) return hipErrorInvalidValue;
    if (a.chunk_rows2 > 64u || (a.chunk_rows2 & (a.chunk_rows2 - 1u)) != 0u) return hipErrorInvalidValue;
    const uint32_t n_tiles = (a.n_rows + 255u) / 256u;
    hipLaunchKernelGGL(attr_mask_kernel, dim3(n_tiles < kMaskGrid ? n_tiles : kMaskGrid), dim3(256), 0, st, a);
    return hipGetLastError();
}

// Work item blockIdx.x is tile (blockIdx.x - item0) of record item_rec[blockIdx.x]: attr_mask_kernel's tile without its counters. A
// wave's 64 rows are two whole words of the record's bitmap; lanes at or beyond n_rows vote false, so the last word's tail is clear.
__global__ __launch_bounds__(256) void attr_mask_pooled_kernel(const AttrMaskRecord* __restrict__ records, const uint32_t* __restrict__ item_rec,
                                                               uint32_t* __restrict__ bitmaps) {
    const AttrMaskRecord r = records[item_rec[blockIdx.x]];
    const uint32_t n_words = (r.n_rows + 31u) / 32u;
    const int lane = lane_id();
    const uint32_t row = (blockIdx.x - r.item0) * 256u + threadIdx.x;
    bool pass = row < r.n_rows;
    if (pass) {
        const int64_t ts = r.ts != nullptr ? r.ts[row] : 0;
        const uint32_t fl = r.flags != nullptr ? r.flags[row] : 0u;
        pass = attr_row_passes(r.has_after, r.after, r.has_before, r.before, r.deny_flags, ts, fl);
    }
    const unsigned long long b = __ballot(pass);
    const uint32_t w0 = (row - (uint32_t)lane) >> 5;
    uint32_t* bitmap = bitmaps + r.word_off;
    if (lane == 0 && w0 < n_words) bitmap[w0] = (uint32_t)b;
    if (lane == 32 && w0 + 1u < n_words) bitmap[w0 + 1u] = (uint32_t)(b >> 32);
}

hipError_t launch_attr_mask_pooled(const AttrMaskRecord* d_records, const uint32_t* d_item_rec, uint32_t n_items, uint32_t* d_bitmaps, hipStream_t st) {
    if (n_items == 0 || d_records == nullptr || d_item_rec == nullptr || d_bitmaps == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(attr_mask_pooled_kernel, dim3(n_items), dim3(256), 0, st, d_records, d_item_rec, d_bitmaps);
    return hipGetLastError();
}

// ---- attribute columns -> row lists, many records per launch (wax_hip_search_batch_predicate) ----
constexpr int kAttrTiles = (int)(ATTR_ROWS_ITEM / 256u);
static_assert(kAttrTiles * 4 == 64, "the emit kernel scans one (tile, wave) count per lane");

// The wave's votes on its 64 rows of each of the item's 16 tiles: tile t of item i is rows i * 4096 + t * 256 .. + 255 of the record,
// one row per lane, both columns read coalesced. Rows at or beyond n_rows vote false, and so do rows whose bit in r.bitmap is clear
// (null: no bitmap, the form as it was).
__device__ inline void attr_rows_votes(const AttrRowsRecord& r, uint32_t item, unsigned long long (&b)[kAttrTiles]) {
    const uint64_t row0 = (uint64_t)item * ATTR_ROWS_ITEM + threadIdx.x;
#pragma unroll
    for (int t = 0; t < kAttrTiles; ++t) {
        const uint64_t row = row0 + (uint64_t)t * 256u;
        bool pass = row < (uint64_t)r.n_rows;
        if (pass && r.bitmap != nullptr) pass = ((r.bitmap[row >> 5] >> (row & 31u)) & 1u) != 0u;   // a term set's rows: the columns are read for these only
        if (pass) {
            const int64_t ts = r.ts != nullptr ? r.ts[row] : 0;
            const uint32_t fl = r.flags != nullptr ? r.flags[row] : 0u;
            pass = attr_row_passes(r.has_after, r.after, r.has_before, r.before, r.deny_flags, ts, fl);
        }
        b[t] = __ballot(pass);
    }
}

__global__ __launch_bounds__(256) void attr_rows_count_kernel(const AttrRowsRecord* __restrict__ records, const uint32_t* __restrict__ item_rec,
                                                              uint32_t* __restrict__ block_sum) {
    __shared__ uint32_t wave_cnt[4];
    const AttrRowsRecord r = records[item_rec[blockIdx.x]];
    const uint32_t item = blockIdx.x - r.item0;
    unsigned long long b[kAttrTiles];
    attr_rows_votes(r, item, b);
    uint32_t n = 0;                                             // wave-uniform
#pragma unroll
    for (int t = 0; t < kAttrTiles; ++t) n += (uint32_t)__popcll(b[t]);
    if (lane_id() == 0) wave_cnt[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) block_sum[r.block0 + item] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// One workgroup per record: exclusive scan of its items' counts in place, the record's total to counts[count_slot].
__global__ __launch_bounds__(256) void attr_rows_scan_kernel(const AttrRowsRecord* __restrict__ records, uint32_t* block_sum, uint32_t* counts) {
    __shared__ uint32_t wave_sum[4];
    const AttrRowsRecord r = records[blockIdx.x];
    uint32_t* bs = block_sum + r.block0;
    const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < r.n_items; b0 += 256u) {
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t v = i < r.n_items ? bs[i] : 0u;
        uint32_t inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wave_sum[w] = inc;
        __syncthreads();
        uint32_t base = 0, all = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < w) base += wave_sum[j];
            all += wave_sum[j];
        }
        if (i < r.n_items) bs[i] = carry + base + inc - v;
        carry += all;
        __syncthreads();                                        // wave_sum is rewritten by the next chunk
    }
    if (threadIdx.x == 0) counts[r.count_slot] = carry;
}

// The count kernel's items once more: the votes again, then every passing row at its rank. Rows ascend with (tile, wave, lane), so the
// rank of a row is its item's offset + the passing rows of the (tile, wave) pairs before its own + the passing lanes below it.
__global__ __launch_bounds__(256) void attr_rows_emit_kernel(const AttrRowsRecord* __restrict__ records, const uint32_t* __restrict__ item_rec,
                                                             const uint32_t* __restrict__ block_off, uint32_t* __restrict__ rows_out) {
    __shared__ uint32_t cnt[kAttrTiles * 4];                    // [tile][wave]
    const AttrRowsRecord r = records[item_rec[blockIdx.x]];
    const uint32_t item = blockIdx.x - r.item0;
    const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
    unsigned long long b[kAttrTiles];
    attr_rows_votes(r, item, b);
#pragma unroll
    for (int t = 0; t < kAttrTiles; ++t)
        if (lane == 0) cnt[t * 4 + w] = (uint32_t)__popcll(b[t]);
    __syncthreads();
    const uint32_t mine = cnt[lane];                            // 64 (tile, wave) pairs, one per lane, in row order
    uint32_t inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    const uint32_t ex = inc - mine;
    uint32_t* out = rows_out + r.row_off + block_off[r.block0 + item];
    const uint32_t row0 = item * ATTR_ROWS_ITEM + threadIdx.x;  // (a passing row is < n_rows: no wrap)
#pragma unroll
    for (int t = 0; t < kAttrTiles; ++t) {
        const uint32_t off = __shfl(ex, t * 4 + w, 64);
        const unsigned long long m = b[t];
        const uint32_t below = (uint32_t)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if ((m >> lane) & 1ull) out[off + below] = row0 + (uint32_t)t * 256u;
    }
}

hipError_t launch_attr_rows(const AttrRowsRecord* d_records, uint32_t n_records, const uint32_t* d_item_rec, uint32_t n_items, uint32_t* block_sum,
                            uint32_t* rows_out, uint32_t* counts, hipStream_t st) {
    if (n_records == 0 || n_items == 0 || d_records == nullptr || d_item_rec == nullptr || block_sum == nullptr || rows_out == nullptr || counts == nullptr)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(attr_rows_count_kernel, dim3(n_items), dim3(256), 0, st, d_records, d_item_rec, block_sum);
    hipLaunchKernelGGL(attr_rows_scan_kernel, dim3(n_records), dim3(256), 0, st, d_records, block_sum, counts);
    hipLaunchKernelGGL(attr_rows_emit_kernel, dim3(n_items), dim3(256), 0, st, d_records, d_item_rec, block_sum, rows_out);
    return hipGetLastError();
}

template <bool NT>
__device__ inline f32x4 ld16m(const f32x4* p) {
    if (NT) return __builtin_nontemporal_load(p);
    return *p;
}

template <int D4, int GROUP, int METRIC, int UNROLL, bool NT, int CAP>
__global__ __launch_bounds__(SCAN_THREADS) void scan_masked_kernel(MaskedScanArgs a) {
    constexpr int LOADS = D4 / GROUP;       // float4s per lane per row
    constexpr int RPW = WAVE / GROUP;       // rows per wave-wide load
    constexpr int RPC = RPW * UNROLL;       // rows per wave per iteration = the chunk of the skip test
    static_assert(D4 % GROUP == 0, "GROUP must divide D4");
    static_assert((RPC & (RPC - 1)) == 0 && RPC <= 32, "a chunk's bits must sit inside one bitmap word");

    __shared__ int64_t lds[SCAN_WAVES * CAP + SCAN_WAVES + FUSED_MAX_K];

    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const int sub = lane / GROUP;
    const int gl = lane % GROUP;
    const bool owner = (gl == GROUP - 1);
    const uint32_t n = a.n_rows;

    const f32x4* __restrict__ store4 = reinterpret_cast<const f32x4*>(a.store);
    const f32x4* __restrict__ q4 = reinterpret_cast<const f32x4*>(a.query);
    const uint32_t* __restrict__ bitmap = a.bitmap;

    f32x4 q[LOADS];
#pragma unroll
    for (int j = 0; j < LOADS; ++j) q[j] = q4[gl + j * GROUP];

    WaveTopK<CAP> tk;
    tk.init(lds + wave * CAP, a.k);

    const uint32_t nchunks = (n + RPC - 1) / RPC;
    const uint32_t gwave = blockIdx.x * SCAN_WAVES + wave;
    const uint32_t nwaves = gridDim.x * SCAN_WAVES;

    // A chunk's bits are requested one iteration ahead. Read at the top of the chunk's own iteration — the first build — the row loads
    // wait a memory round trip behind them in every iteration, with 8 waves per CU to hide it. That build's masked route was
    // 2.5 x the unfiltered scan with 15/16 passing and nothing skipped (profiles/r13/c_routes_first_build.json); how much of that
    // was this dependency was not measured on its own.
    uint32_t word = gwave < nchunks ? bitmap[(gwave * RPC) >> 5] : 0u;
    for (uint32_t chunk = gwave; chunk < nchunks; chunk += nwaves) {
        const uint32_t r0 = chunk * RPC;                     // < n: word r0 >> 5 exists; bits of rows >= n are clear
        const uint32_t bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)((word >> (r0 & 31u)) & (uint32_t)((1ull << RPC) - 1ull)));
        const uint32_t next = chunk + nwaves;
        if (next < nchunks) word = bitmap[(next * RPC) >> 5];
        if (bits == 0u) continue;                            // wave-uniform: no row of the chunk may be offered, so none is loaded
        const uint32_t rbase = r0 + sub;
        tk.make_room(RPC);
        f32x4 v[UNROLL][LOADS];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const uint32_t r = rbase + u * RPW;
            const uint32_t rc = r < n ? r : n - 1;  // clamp: tail lanes re-read the last row, result discarded
            const f32x4* p = store4 + (size_t)rc * D4 + gl;
#pragma unroll
            for (int j = 0; j < LOADS; ++j) v[u][j] = ld16m<NT>(p + j * GROUP);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f}, nrm = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < LOADS; ++j) accumulate<METRIC>(q[j], v[u][j], acc, nrm);
            const float d = finish_row<GROUP, METRIC>(acc, nrm, a.q_norm);
            const uint32_t r = rbase + u * RPW;
            const bool valid = owner && (r < n) && ((bits >> (uint32_t)(sub + u * RPW)) & 1u) != 0u;
            tk.push(make_key(d, a.row_base + r), valid);
        }
    }

    int* counts = reinterpret_cast<int*>(lds + SCAN_WAVES * CAP);
    int64_t* fin = lds + SCAN_WAVES * CAP + SCAN_WAVES;
    tk.finalize();
    if (lane == 0) counts[wave] = tk.cnt;
    __syncthreads();
    block_rank_merge<SCAN_WAVES>(lds, CAP, counts, a.k, fin);
    __syncthreads();
    int64_t* mine = a.partials + (size_t)blockIdx.x * a.k;
    for (int t = (int)threadIdx.x; t < a.k; t += SCAN_THREADS) mine[t] = fin[t];
}

// Row groups in flight per wave: the f32 scan's at 384-d and 768-d (kernels.hip), elsewhere the nearest power of two, so that a
// chunk is an aligned run of 2 .. 16 rows whose bits never straddle a bitmap word. Speed only: the lanes per row fix the bits.
template <typename S>
static constexpr int masked_unroll() {
    return S::DIMS == 768 ? 2 : (S::LOADS <= 3 ? 4 : 2);
}

bool scan_masked_dims(uint32_t dims) { return scan_group_lanes(dims) != 0; }

uint32_t scan_masked_chunk_rows(uint32_t dims) {
    return with_scan_shape(dims, [](auto s) {
        using S = decltype(s);
        return (uint32_t)((WAVE / S::GROUP) * masked_unroll<S>());
    }, 0u);
}

hipError_t launch_scan_masked(const MaskedScanArgs& a, int metric, int cap, int grid_cap, hipStream_t st, int* out_grid) {
    if (a.k < 1 || a.k > FUSED_MAX_K || a.n_rows == 0 || a.bitmap == nullptr || a.query == nullptr || a.partials == nullptr)
        return hipErrorInvalidValue;
    if (a.k > 64 && cap <= 128) return hipErrorInvalidValue;
    const int grid = scan_grid_for(a.n_rows, a.dims, 0, grid_cap);
    if (out_grid) *out_grid = grid;
    return with_scan_shape(a.dims, [&](auto s) {
        using S = decltype(s);
        constexpr int U = masked_unroll<S>();
        return with_metric(metric, [&](auto m) {
            constexpr int M = decltype(m)::value;
            if (cap <= 128) hipLaunchKernelGGL((scan_masked_kernel<S::D4, S::GROUP, M, U, true, 128>), dim3(grid), dim3(SCAN_THREADS), 0, st, a);
            else hipLaunchKernelGGL((scan_masked_kernel<S::D4, S::GROUP, M, U, true, 256>), dim3(grid), dim3(SCAN_THREADS), 0, st, a);
            return hipGetLastError();
        }, hipErrorInvalidValue);
    }, hipErrorInvalidValue);
}

}  // namespace wax
