// filter.hip — device side of the allow-list pre-filter of wax_hip_search_filtered (SURVEY.md §8f-4;
// FrameFilter.frameIds, UnifiedSearch.swift:1241-1258): frame ids -> rows of the store without a host probe per id.
//
//   idhash_build_kernel    id -> row open-addressing table in HBM (u32 slots holding row+1, 0 = empty; linear probing).
//                          Rebuilt lazily after a mutation, like the bf16 mirror. 4 bytes per slot, load factor <= 0.5.
//   idhash_probe_kernel    one thread per allowed id: probe, mark the row in a bitmap (atomicOr). The bitmap hands the
//                          rows back ascending and unique — the order every selection path breaks ties in.
//   bitmap_count / bitmap_scan / bitmap_emit   bitmap -> compact ascending row list + the rows' frame ids.
//   rowlist_sort_kernel    batched filtered search: one workgroup per allow-list of <= ROWLIST_SORT_MAX ids probes, sorts the
//                          rows in LDS (bitonic) and writes them ascending and unique with a device-side count. PRED = true
//                          (batched predicates) drops the probed rows that fail the list's row predicate before the sort.
//
// All HBM-latency work: at a 1M-id allow-list the probes are ~2M random 64-byte sector reads, a few tens of µs on the
// device against 5.65 ms of cache-missing host probes (profiles/r01).
#include "kernels.h"

namespace wax {

__device__ __forceinline__ uint64_t mix64(uint64_t x) {  // splitmix64 finaliser
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

__global__ __launch_bounds__(256) void idhash_build_kernel(const uint64_t* __restrict__ ids, uint32_t row0, uint32_t n, uint32_t* table,
                                                           uint32_t mask) {
    const uint32_t row = row0 + blockIdx.x * 256u + threadIdx.x;     // rows [row0, n): the appended ones, or all of them (row0 = 0)
    if (row >= n) return;
    uint32_t h = (uint32_t)mix64(ids[row]) & mask;
    while (atomicCAS(&table[h], 0u, row + 1u) != 0u) h = (h + 1u) & mask;
}

constexpr uint32_t kNoRow = 0xffffffffu;

// The row of frame id `id`, kNoRow if the store does not hold it.
__device__ __forceinline__ uint32_t idhash_lowest_row(uint64_t id, const uint64_t* __restrict__ ids, const uint32_t* __restrict__ table,
                                                      uint32_t mask) {
    uint32_t h = (uint32_t)mix64(id) & mask;
    // A store loaded from a segment may hold one frame id in several rows (deserialize keeps them as separate rows and the
    // host id map resolves the id to the FIRST of them, MetalVectorEngine.swift:809-811 / firstIndex(of:)). All rows of
    // one id sit in the same probe chain, in whatever order the build's CAS races left them: walk the chain to its end
    // and mark the LOWEST matching row, so the device path picks the row the host path picks, on every run.
    uint32_t best = kNoRow;
    for (;;) {
        const uint32_t s = table[h];
        if (s == 0u) break;   // end of the chain (an allowed id without a vector is simply absent, UnifiedSearch.swift:1243)
        if (ids[s - 1u] == id && s - 1u < best) best = s - 1u;
        h = (h + 1u) & mask;
    }
    return best;
}

__global__ __launch_bounds__(256) void idhash_probe_kernel(const uint64_t* __restrict__ allow, uint64_t n_allow,
                                                           const uint64_t* __restrict__ ids, const uint32_t* __restrict__ table,
                                                           uint32_t mask, uint32_t* bitmap) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_allow) return;
    const uint32_t best = idhash_lowest_row(allow[i], ids, table, mask);
    if (best != kNoRow) atomicOr(&bitmap[best >> 5], 1u << (best & 31u));
}

// One workgroup per list: probe every id into LDS (kNoRow for an id the store lacks), bitonic sort of the next power of two,
// then keep the first of every run of equal rows (duplicate ids) and drop kNoRow; a workgroup-wide scan places the survivors.
// PRED (wax_hip_search_batch_predicate): list blockIdx.x carries the row predicate preds[blockIdx.x]; a probed row that fails it
// — or, where the entry has required terms (n_terms != 0), lacks one of them in its row of the CSR term column —
// becomes kNoRow before the sort. PRED = false never reads `preds` and is the kernel of the lists without a predicate.
constexpr int kSortThreads = 1024;
template <bool PRED>
__global__ __launch_bounds__(kSortThreads) void rowlist_sort_kernel(const uint64_t* __restrict__ allow, const RowListDesc* __restrict__ desc,
                                                                    const uint64_t* __restrict__ ids, const uint32_t* __restrict__ table,
                                                                    uint32_t mask, uint32_t* __restrict__ rows_out, uint32_t* counts,
                                                                    const RowListPred* __restrict__ preds) {
    extern __shared__ uint32_t srt[];              // [P]
    __shared__ uint32_t wave_sum[kSortThreads / 64];
    const RowListDesc d = desc[blockIdx.x];
    const uint32_t t = threadIdx.x;
    uint32_t P = 64;
    while (P < d.len) P <<= 1;                     // len <= ROWLIST_SORT_MAX (host-checked)
    if constexpr (PRED) {
        const RowListPred p = preds[blockIdx.x];
        for (uint32_t i = t; i < P; i += kSortThreads) {
            uint32_t row = i < d.len ? idhash_lowest_row(allow[d.allow_off + i], ids, table, mask) : kNoRow;
            if (row != kNoRow) {
                const int64_t ts = p.ts != nullptr ? p.ts[row] : 0;
                const uint32_t fl = p.flags != nullptr ? p.flags[row] : 0u;
                if (!attr_row_passes(p.has_after, p.after, p.has_before, p.before, p.deny_flags, ts, fl)) row = kNoRow;
            }
            if (row != kNoRow && p.n_terms != 0u) {
                // the required terms of the list's queries (wax_hip_search_batch_terms): term_mask_kernel's test on this one row
                const uint32_t end = p.term_off[row + 1u];
                uint32_t bits = 0u;
                for (uint32_t v = p.term_off[row]; v < end; ++v) {
                    const uint32_t x = p.term_val[v];
#pragma unroll
                    for (int j = 0; j < 16; ++j) bits |= x == p.terms[j] ? (1u << j) : 0u;
                }
                if (bits != 0xffffu) row = kNoRow;
            }
            srt[i] = row;
        }
    } else {
        for (uint32_t i = t; i < P; i += kSortThreads) srt[i] = i < d.len ? idhash_lowest_row(allow[d.allow_off + i], ids, table, mask) : kNoRow;
    }
    __syncthreads();
    for (uint32_t kk = 2; kk <= P; kk <<= 1) {
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            for (uint32_t i = t; i < P; i += kSortThreads) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const uint32_t x = srt[i], y = srt[l];
                    if ((x > y) == ((i & kk) == 0)) { srt[i] = y; srt[l] = x; }
                }
            }
            __syncthreads();
        }
    }
    const int lane = (int)(t & 63u), w = (int)(t >> 6);
    uint32_t base = 0;
    for (uint32_t c0 = 0; c0 < P; c0 += kSortThreads) {
        const uint32_t i = c0 + t;
        const uint32_t v = i < P ? srt[i] : kNoRow;
        const bool keep = v != kNoRow && (i == 0 || srt[i - 1] != v);
        const unsigned long long m = __ballot(keep);
        const uint32_t before = (uint32_t)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (lane == 0) wave_sum[w] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t off = 0, all = 0;
        for (int j = 0; j < kSortThreads / 64; ++j) {
            if (j < w) off += wave_sum[j];
            all += wave_sum[j];
        }
        if (keep) rows_out[d.row_off + base + off + before] = v;
        base += all;
        __syncthreads();                           // wave_sum is rewritten by the next chunk
    }
    if (t == 0) counts[d.count_slot] = base;
}

constexpr int kWordsPerThread = 4;
constexpr int kWordsPerBlock = 256 * kWordsPerThread;

__device__ __forceinline__ uint32_t block_exclusive_scan_256(uint32_t v, uint32_t* total) {
    __shared__ uint32_t wave_sum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
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
    *total = all;
    __syncthreads();
    return base + inc - v;
}

__global__ __launch_bounds__(256) void bitmap_count_kernel(const uint32_t* __restrict__ bitmap, uint32_t n_words,
                                                           uint32_t* block_sum) {
    const uint32_t w0 = blockIdx.x * kWordsPerBlock + threadIdx.x * kWordsPerThread;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < kWordsPerThread; ++j)
        if (w0 + j < n_words) c += __popc(bitmap[w0 + j]);
    uint32_t total;
    (void)block_exclusive_scan_256(c, &total);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// One workgroup: exclusive scan of block_sum in place, grand total to *total.
__global__ __launch_bounds__(256) void bitmap_scan_kernel(uint32_t* block_sum, uint32_t n_blocks, uint32_t* total) {
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += 256u) {
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t v = i < n_blocks ? block_sum[i] : 0u;
        uint32_t chunk;
        const uint32_t ex = block_exclusive_scan_256(v, &chunk);
        if (i < n_blocks) block_sum[i] = carry + ex;
        carry += chunk;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(256) void bitmap_emit_kernel(const uint32_t* __restrict__ bitmap, uint32_t n_words,
                                                          const uint32_t* __restrict__ block_off, const uint64_t* __restrict__ ids,
                                                          uint32_t* rows_out, uint64_t* ids_out) {
    const uint32_t w0 = blockIdx.x * kWordsPerBlock + threadIdx.x * kWordsPerThread;
    uint32_t words[kWordsPerThread];
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < kWordsPerThread; ++j) {
        words[j] = w0 + j < n_words ? bitmap[w0 + j] : 0u;
        c += __popc(words[j]);
    }
    uint32_t total;
    uint32_t pos = block_off[blockIdx.x] + block_exclusive_scan_256(c, &total);
#pragma unroll
    for (int j = 0; j < kWordsPerThread; ++j) {
        uint32_t w = words[j];
        while (w) {
            const uint32_t row = (w0 + j) * 32u + (uint32_t)__builtin_ctz(w);
            rows_out[pos] = row;
            ids_out[pos] = ids[row];
            ++pos;
            w &= w - 1u;
        }
    }
}

hipError_t launch_idhash_build(const uint64_t* ids, uint32_t row0, uint32_t n, uint32_t* table, uint64_t slots, hipStream_t st) {
    hipError_t err = hipSuccess;
    if (row0 == 0) err = hipMemsetAsync(table, 0, (size_t)slots * sizeof(uint32_t), st);   // from scratch; row0 > 0 inserts into the live table
    if (err != hipSuccess || n <= row0) return err;
    hipLaunchKernelGGL(idhash_build_kernel, dim3((n - row0 + 255u) / 256u), dim3(256), 0, st, ids, row0, n, table, (uint32_t)(slots - 1));
    return hipGetLastError();
}

uint32_t filter_bitmap_blocks(uint32_t n_rows) {
    const uint32_t n_words = (n_rows + 31u) / 32u;
    return (n_words + (uint32_t)kWordsPerBlock - 1u) / (uint32_t)kWordsPerBlock;
}

hipError_t launch_bitmap_offsets(const uint32_t* bitmap, uint32_t n_rows, uint32_t* block_sum, uint32_t* total, hipStream_t st) {
    const uint32_t n_words = (n_rows + 31u) / 32u;
    const uint32_t n_blocks = filter_bitmap_blocks(n_rows);
    hipLaunchKernelGGL(bitmap_count_kernel, dim3(n_blocks), dim3(256), 0, st, bitmap, n_words, block_sum);
    hipLaunchKernelGGL(bitmap_scan_kernel, dim3(1), dim3(256), 0, st, block_sum, n_blocks, total);
    return hipGetLastError();
}

hipError_t launch_allow_probe(const uint64_t* d_allow, uint64_t n_allow, const uint64_t* ids, uint32_t n_rows,
                              const uint32_t* table, uint64_t slots, uint32_t* bitmap, uint32_t* block_sum, uint32_t* total,
                              hipStream_t st) {
    const uint32_t n_words = (n_rows + 31u) / 32u;
    hipError_t err = hipMemsetAsync(bitmap, 0, (size_t)n_words * sizeof(uint32_t), st);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(idhash_probe_kernel, dim3((unsigned)((n_allow + 255u) / 256u)), dim3(256), 0, st, d_allow, n_allow, ids,
                       table, (uint32_t)(slots - 1), bitmap);
    if (block_sum == nullptr) return hipGetLastError();   // the caller finishes the bitmap first (predicate search) and asks for the offsets then
    return launch_bitmap_offsets(bitmap, n_rows, block_sum, total, st);
}

hipError_t launch_rowlist_sort(const uint64_t* d_allow, const RowListDesc* d_desc, const RowListPred* d_preds, uint32_t n_lists, uint32_t max_len,
                               const uint64_t* ids, const uint32_t* table, uint64_t slots, uint32_t* rows_out, uint32_t* counts, hipStream_t st) {
    if (n_lists == 0) return hipSuccess;
    if (max_len > ROWLIST_SORT_MAX) return hipErrorInvalidValue;
    uint32_t P = 64;
    while (P < max_len) P <<= 1;
    const size_t smem = (size_t)P * sizeof(uint32_t);
    static std::atomic<uint64_t> configured{0}, configured_pred{0};   // per device (ensure_dynamic_lds), per instantiation
    if (smem > 64 * 1024 - 256) {
        const hipError_t e = d_preds ? ensure_dynamic_lds(reinterpret_cast<const void*>(&rowlist_sort_kernel<true>), 96 * 1024, configured_pred)
                                     : ensure_dynamic_lds(reinterpret_cast<const void*>(&rowlist_sort_kernel<false>), 96 * 1024, configured);
        if (e != hipSuccess) return e;
    }
    if (d_preds)
        hipLaunchKernelGGL(rowlist_sort_kernel<true>, dim3(n_lists), dim3(kSortThreads), smem, st, d_allow, d_desc, ids, table,
                           (uint32_t)(slots - 1), rows_out, counts, d_preds);
    else
        hipLaunchKernelGGL(rowlist_sort_kernel<false>, dim3(n_lists), dim3(kSortThreads), smem, st, d_allow, d_desc, ids, table,
                           (uint32_t)(slots - 1), rows_out, counts, d_preds);
    return hipGetLastError();
}

hipError_t launch_allow_emit(const uint32_t* bitmap, uint32_t n_rows, const uint32_t* block_off, const uint64_t* ids,
                             uint32_t* rows_out, uint64_t* ids_out, hipStream_t st) {
    const uint32_t n_words = (n_rows + 31u) / 32u;
    hipLaunchKernelGGL(bitmap_emit_kernel, dim3(filter_bitmap_blocks(n_rows)), dim3(256), 0, st, bitmap, n_words, block_off, ids,
                       rows_out, ids_out);
    return hipGetLastError();
}

}  // namespace wax
