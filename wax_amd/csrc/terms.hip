// terms.hip — device side of wax_hip_search_terms (FrameFilter.metadataFilter, SearchRequest.swift:130-145;
// matches(metadataFilter:meta:), UnifiedSearch.swift:1215-1239): the CSR term column -> the row bitmap every filter route works from.
//
//   term_mask_kernel       the product: one lane per row. A lane walks its own row's values (one dword per lane and iteration; the wave
//                          runs as long as its longest set), matches each against the sixteen required terms (wave-uniform scalars:
//                          a compare chain), and one ballot writes the two bitmap words, as attr_mask_kernel does (which runs behind
//                          this kernel with and_bitmap = 1 and does all the counting). No LDS, no atomics. One workgroup per 256 rows
//                          up to WAX_TERM_MASK_GRID_CAP, grid-strided beyond.
//   term_mask_wave_kernel  the wave-cooperative form, kept as the measured alternative (-DWAX_TERM_MASK_FORM=0 launches it in the
//                          product's place): a wave owns 64 consecutive rows, stages their 65 offsets in LDS and streams the
//                          CONTIGUOUS span values[off[r0] .. off[r0 + 64]) with dwordx4 loads, TERM_MASK_PIECE values (four loads per
//                          lane) per iteration; only a value that IS a required term bisects the 65 offsets for its row and ORs its
//                          bit into the row's LDS word; lane i then tests row i's word. At 10M rows x 6 terms it takes 183 us where
//                          the product takes 81: two dependent loads per 64 rows and little in flight per wave. Sets
//                          near 64 terms, where a lane-per-row wave is serialised by its longest set, are not measured.
//   term_mask_multi_kernel the batched form's (wax_hip_search_batch_terms): the lane-per-row walk once for up to 32 term sets — the
//                          sets' union and membership words in LDS, a bit-sliced 5-bit counter per set and row, one bitmap and one
//                          passing count per set (below).
#include "kernels.h"
#include "topk.h"

namespace wax {

constexpr uint32_t kTermLoads = TERM_MASK_PIECE / 256u;      // dwordx4 loads per lane and iteration
static_assert(kTermLoads * 256u == TERM_MASK_PIECE, "a piece is whole dwordx4 loads of 64 lanes");

__global__ __launch_bounds__(256) void term_mask_wave_kernel(TermMaskArgs a) {
    __shared__ uint32_t s_off[4][65];
    __shared__ uint32_t s_hit[4][64];
    const uint32_t n_words = (a.n_rows + 31u) / 32u;
    const uint32_t n_groups = (a.n_rows + 63u) / 64u;
    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    uint32_t* off_s = s_off[wave];
    uint32_t* hit_s = s_hit[wave];
    for (uint32_t g = blockIdx.x * 4u + (uint32_t)wave; g < n_groups; g += gridDim.x * 4u) {
        const uint32_t r0 = g * 64u;
        const uint32_t row = r0 + (uint32_t)lane;
        // rows at and beyond n_rows read off[n_rows]: empty sets at the end of the span
        off_s[lane] = a.off[row < a.n_rows ? row : a.n_rows];
        if (lane == 0) off_s[64] = a.off[r0 + 64u < a.n_rows ? r0 + 64u : a.n_rows];
        hit_s[lane] = 0u;
        wave_lds_fence();
        const uint32_t begin = (uint32_t)__builtin_amdgcn_readfirstlane((int)off_s[0]);
        const uint32_t end = (uint32_t)__builtin_amdgcn_readfirstlane((int)off_s[64]);
        // positions are counted from the 16-byte boundary at or below `begin`: rel < span <= 64 * 64 + 3 however large the column is
        const uint32_t lead = begin & 3u;
        const uint32_t span = end - begin + lead;
        const uint32_t* __restrict__ base = a.val + (begin - lead);
        for (uint32_t done = 0; done < span; done += TERM_MASK_PIECE) {
            uint4 v[kTermLoads];
#pragma unroll
            for (uint32_t u = 0; u < kTermLoads; ++u) {
                const uint32_t rel = done + (u * 64u + (uint32_t)lane) * 4u;
                v[u] = rel < span ? *reinterpret_cast<const uint4*>(base + rel) : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (uint32_t u = 0; u < kTermLoads; ++u) {
                const uint32_t rel = done + (u * 64u + (uint32_t)lane) * 4u;
                const uint32_t x[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j) {
                    uint32_t bits = 0u;
#pragma unroll
                    for (int i = 0; i < TERMS_MAX_REQUIRED; ++i) bits |= x[j] == a.req[i] ? (1u << i) : 0u;
                    const uint32_t p = rel + j;
                    if (bits != 0u && p >= lead && p < span) {
                        const uint32_t pos = begin - lead + p;      // off_s[lo] <= pos < off_s[hi] throughout
                        uint32_t lo = 0u, hi = 64u;
#pragma unroll
                        for (int s = 0; s < 6; ++s) {
                            const uint32_t mid = (lo + hi) >> 1;
                            if (off_s[mid] <= pos) lo = mid; else hi = mid;
                        }
                        atomicOr(&hit_s[lo], bits);
                    }
                }
            }
        }
        wave_lds_fence();
        bool pass = row < a.n_rows && hit_s[lane] == 0xffffu;
        if (pass && a.and_bitmap != 0) pass = ((a.bitmap[row >> 5] >> (row & 31u)) & 1u) != 0u;   // (read by the wave that rewrites the word below)
        const unsigned long long b = __ballot(pass);
        const uint32_t w0 = r0 >> 5;
        if (lane == 0 && w0 < n_words) a.bitmap[w0] = (uint32_t)b;
        if (lane == 32 && w0 + 1u < n_words) a.bitmap[w0 + 1u] = (uint32_t)(b >> 32);
        wave_lds_fence();                                       // the next group's offsets overwrite what the bisection read
    }
}

// The product's form (1) or the wave-cooperative one (0); the product's own grid.
#ifndef WAX_TERM_MASK_FORM
#define WAX_TERM_MASK_FORM 1
#endif
#ifndef WAX_TERM_MASK_GRID_CAP                 // the product's own grid: one workgroup per 256 rows up to this many, grid-strided beyond
#define WAX_TERM_MASK_GRID_CAP 16384
#endif
__global__ __launch_bounds__(256) void term_mask_kernel(TermMaskArgs a) {
    const uint32_t n_words = (a.n_rows + 31u) / 32u;
    const uint32_t n_tiles = (a.n_rows + 255u) / 256u;
    const int lane = lane_id();
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t row = tile * 256u + threadIdx.x;
        bool pass = false;
        if (row < a.n_rows) {
            const uint32_t end = a.off[row + 1u];
            uint32_t bits = 0u;
            for (uint32_t p = a.off[row]; p < end; ++p) {
                const uint32_t x = a.val[p];
#pragma unroll
                for (int i = 0; i < TERMS_MAX_REQUIRED; ++i) bits |= x == a.req[i] ? (1u << i) : 0u;
            }
            pass = bits == 0xffffu;
            if (pass && a.and_bitmap != 0) pass = ((a.bitmap[row >> 5] >> (row & 31u)) & 1u) != 0u;
        }
        const unsigned long long b = __ballot(pass);
        const uint32_t w0 = (row - (uint32_t)lane) >> 5;
        if (lane == 0 && w0 < n_words) a.bitmap[w0] = (uint32_t)b;
        if (lane == 32 && w0 + 1u < n_words) a.bitmap[w0 + 1u] = (uint32_t)(b >> 32);
    }
}

hipError_t launch_term_mask(const TermMaskArgs& a, uint32_t grid, hipStream_t st) {
    if (a.n_rows == 0 || a.off == nullptr || a.bitmap == nullptr || grid > TERM_MASK_MAX_GRID) return hipErrorInvalidValue;
    if (a.val == nullptr || (reinterpret_cast<uintptr_t>(a.val) & 15u) != 0u) return hipErrorInvalidValue;
    if (grid == 0) {
        const uint32_t n_tiles = (a.n_rows + 255u) / 256u;
        grid = n_tiles < (uint32_t)WAX_TERM_MASK_GRID_CAP ? n_tiles : (uint32_t)WAX_TERM_MASK_GRID_CAP;
    }
#if WAX_TERM_MASK_FORM == 0
    hipLaunchKernelGGL(term_mask_wave_kernel, dim3(grid), dim3(256), 0, st, a);
#else
    hipLaunchKernelGGL(term_mask_kernel, dim3(grid), dim3(256), 0, st, a);
#endif
    return hipGetLastError();
}

// ---- up to 32 term sets in one pass over the column (wax_hip_search_batch_terms) ----
// term_mask_kernel's lane-per-row walk, but a value is looked up once for all the sets: the sorted union of their terms and one
// membership word per term sit in LDS (padded to 512 entries with UINT32_MAX / 0), a value inside [first, last] of the union bisects it
// without a branch (log2 of the padded size steps), and its membership word m is ADDED to five bit-sliced words c0..c4 — bit s of
// (c4..c0) is a 5-bit counter of the terms of set s the row holds. Row values are distinct and so are a set's terms, so counter s never
// exceeds |set s| <= 16 and a row passes set s exactly when the counter equals |set s| (nbits). One ballot per set writes the set's two
// bitmap words; lane s of every wave keeps the count of set s, and a workgroup adds its 32 counts once at the end.
#ifndef WAX_TERM_MULTI_GRID_CAP
#define WAX_TERM_MULTI_GRID_CAP 2048
#endif
__global__ __launch_bounds__(256) void term_mask_multi_kernel(TermMaskMultiArgs a) {
    __shared__ uint32_t s_u[TERM_MULTI_MAX_UNION];
    __shared__ uint32_t s_m[TERM_MULTI_MAX_UNION];
    __shared__ uint32_t s_cnt[4][TERM_MULTI_MAX_SETS];
    for (uint32_t i = threadIdx.x; i < TERM_MULTI_MAX_UNION; i += 256u) { s_u[i] = a.uni[i]; s_m[i] = a.memb[i]; }
    __syncthreads();
    const uint32_t n_words = (a.n_rows + 31u) / 32u;
    const uint32_t n_tiles = (a.n_rows + 255u) / 256u;
    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const uint32_t first = s_u[0], last = s_u[a.n_union - 1u];
    uint32_t top = 1u;                                          // half of the padded size: the first bisection step
    while (top * 2u < a.n_union) top <<= 1;                     // n_union <= 2 * top <= 512
    const uint32_t live = a.n_sets >= 32u ? 0xffffffffu : (1u << a.n_sets) - 1u;
    const uint32_t n0 = a.nbits[0], n1 = a.nbits[1], n2 = a.nbits[2], n3 = a.nbits[3], n4 = a.nbits[4];
    uint32_t my_count = 0;                                      // lane s (and s + 32: unused) of every wave: rows of this wave that pass set s
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t row = tile * 256u + threadIdx.x;
        uint32_t pass = 0u;
        if (row < a.n_rows) {
            const uint32_t end = a.off[row + 1u];
            uint32_t c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u, c4 = 0u;
            for (uint32_t p = a.off[row]; p < end; ++p) {
                const uint32_t x = a.val[p];
                if (x < first || x > last) continue;
                uint32_t lo = 0u;                               // the number of union terms below x, at most 2 * top - 1
                for (uint32_t s = top; s != 0u; s >>= 1) lo += s_u[lo + s - 1u] < x ? s : 0u;
                uint32_t carry = s_u[lo] == x ? s_m[lo] : 0u;
                uint32_t t;
                t = c0 & carry; c0 ^= carry; carry = t;
                t = c1 & carry; c1 ^= carry; carry = t;
                t = c2 & carry; c2 ^= carry; carry = t;
                t = c3 & carry; c3 ^= carry; carry = t;
                c4 ^= carry;
            }
            pass = ~((c0 ^ n0) | (c1 ^ n1) | (c2 ^ n2) | (c3 ^ n3) | (c4 ^ n4)) & live;
        }
        const uint32_t w0 = (row - (uint32_t)lane) >> 5;        // the wave's 64 rows are words w0, w0 + 1 of every bitmap
        for (uint32_t s = 0; s < a.n_sets; ++s) {
            const unsigned long long b = __ballot(((pass >> s) & 1u) != 0u);
            uint32_t* bm = a.bitmaps + (size_t)s * a.stride_words;
            if (lane == 0 && w0 < n_words) bm[w0] = (uint32_t)b;
            if (lane == 32 && w0 + 1u < n_words) bm[w0 + 1u] = (uint32_t)(b >> 32);
            if ((uint32_t)lane == s) my_count += (uint32_t)__popcll(b);
        }
    }
    if (lane < (int)TERM_MULTI_MAX_SETS) s_cnt[wave][lane] = my_count;
    __syncthreads();
    if (threadIdx.x < a.n_sets) {
        const uint32_t v = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
        if (v != 0u) atomicAdd(&a.counts[threadIdx.x], v);
    }
}

hipError_t launch_term_mask_multi(const TermMaskMultiArgs& a, uint32_t grid, hipStream_t st) {
    if (a.n_rows == 0 || a.off == nullptr || a.val == nullptr || a.uni == nullptr || a.memb == nullptr || a.bitmaps == nullptr || a.counts == nullptr)
        return hipErrorInvalidValue;
    if (a.n_sets == 0 || a.n_sets > TERM_MULTI_MAX_SETS || a.n_union == 0 || a.n_union > TERM_MULTI_MAX_UNION) return hipErrorInvalidValue;
    if (a.stride_words < (a.n_rows + 31u) / 32u || grid > TERM_MASK_MAX_GRID) return hipErrorInvalidValue;
    if (grid == 0) {
        const uint32_t n_tiles = (a.n_rows + 255u) / 256u;
        grid = n_tiles < (uint32_t)WAX_TERM_MULTI_GRID_CAP ? n_tiles : (uint32_t)WAX_TERM_MULTI_GRID_CAP;
    }
    hipLaunchKernelGGL(term_mask_multi_kernel, dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace wax
