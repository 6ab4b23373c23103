// mirror_wide.hip — the finish of ONE query for 32 < k <= MIRROR_WIDE_MAX_K behind a pass over either mirror ("The wide
// finish"). The passes (mirror_scan.hip, mirror8_scan.hip) are unchanged: each workgroup leaves its MIRROR_KP smallest approximate
// keys, sorted, whatever k is. mirror_finish takes 64 candidates from those lists, which cannot certify k > 16 on the code mirror;
// here up to C = 1 024 or 4 096 are taken, under a bound that keeps the argument of the certificate whole.
//
//   select   mirror_wide_select_kernel, one workgroup of 1 024 threads. Every listed key is read ONCE, 32 per thread, and stays in
//            registers (up to 512 lists x 64 keys = 256 KB: too much for LDS, 64 VGPRs per thread). With T the smallest last key of a
//            full list and K_C the listed key of rank C, B = min(T, K_C): a row a workgroup did not list has a key >= that
//            workgroup's last key >= T, and a listed key that is no candidate is >= B by construction — every row that is not a
//            candidate has a key >= B. T is one reduction over the lanes that hold list tails; K_C is only needed when more than C
//            listed keys lie below T, and is then a radix select over the registers: 11-bit digits from the highest bit in which
//            two live keys differ (the bits above it are shared: no pass is spent on them and no histogram bin takes every key),
//            LDS histogram, one workgroup scan per digit. The candidates are compacted with one LDS counter per wave ballot.
//   rescore  mirror_wide_rescore_kernel, C / (rows per workgroup) workgroups: a lane group per candidate, FLIGHT rows of a wave in
//            flight before the first product, row_distance at ScanShape<DIMS> — the f32 scan's bits.
//   finish   mirror_wide_finish_kernel, one workgroup: bitonic sort of the exact keys in LDS (<= 32 KB), the kpad hits with frame
//            ids, the certificate. Certified iff B == KEY_PAD (every row was re-scored) or dist(B) - eps > d_k, strict, all finite,
//            m >= k, the query's norm not NaN: a row outside the candidates has exact distance >= (its key's distance) - eps >=
//            dist(B) - eps > d_k, so the k best of the candidates are the k best of the store.
#include <cstddef>
#include <cstring>

#include "kernels.h"
#include "mirror_finish.h"

namespace wax {

namespace {

constexpr int WIDE_THREADS = MERGE_THREADS, WIDE_WAVES = MERGE_WAVES;
constexpr int WIDE_KEYS = SCAN_KWAY_MERGE_GRID * MIRROR_KP / WIDE_THREADS;   // listed keys per thread: 32
constexpr int WIDE_DIGIT = 11, WIDE_BINS = 1 << WIDE_DIGIT;                  // two bins per thread
constexpr uint64_t WIDE_SIGN = 0x8000000000000000ull;
constexpr uint64_t WIDE_UPAD = ~0ull;                                        // KEY_PAD in unsigned order
static_assert(WIDE_KEYS * WIDE_THREADS == SCAN_KWAY_MERGE_GRID * MIRROR_KP && WIDE_BINS == 2 * WIDE_THREADS, "the select's shape");
static_assert(WIDE_THREADS % MIRROR_KP == 0, "a list's last key sits in lane 63");

// signed key order as unsigned order and back
__device__ __forceinline__ uint64_t wide_u(int64_t key) { return (uint64_t)key ^ WIDE_SIGN; }
__device__ __forceinline__ int64_t wide_key(uint64_t u) { return (int64_t)(u ^ WIDE_SIGN); }
// the bits of x at and above position `top` (top = 64: none)
__device__ __forceinline__ uint64_t wide_above(uint64_t x, int top) { return top >= 64 ? 0ull : x >> top; }

// op over the workgroup's values, in every thread (red: WIDE_WAVES words, reusable at once by the next call)
template <class OP>
__device__ __forceinline__ uint64_t wide_reduce(uint64_t v, uint64_t* red, OP op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, (uint64_t)__shfl_xor((unsigned long long)v, o));
    __syncthreads();
    if (lane_id() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t r = red[0];
#pragma unroll
    for (int w = 1; w < WIDE_WAVES; ++w) r = op(r, red[w]);
    return r;
}

}  // namespace

__global__ __launch_bounds__(WIDE_THREADS) void mirror_wide_select_kernel(const int64_t* __restrict__ lists_keys, int lists, int c,
                                                                          int64_t* __restrict__ cand, uint64_t* __restrict__ ctl) {
    __shared__ uint32_t hist[WIDE_BINS];
    __shared__ uint64_t red[WIDE_WAVES];
    __shared__ uint32_t wave_total[WIDE_WAVES];
    __shared__ uint64_t pick[2];                 // the digit's choice: the key's bits so far, the rank left inside them
    __shared__ uint32_t fill;
    const int t = (int)threadIdx.x, lane = lane_id(), wave = t >> 6;
    const int n = lists * MIRROR_KP;
    // one workgroup per member: member b's lists, candidates and control words lie b whole sets behind the first member's
    lists_keys += (size_t)blockIdx.x * n;
    cand += (size_t)blockIdx.x * c;
    ctl += (size_t)blockIdx.x * MIRROR_WIDE_CTL;

    // (1) the listed keys, once: key i = j * WIDE_THREADS + t, so slot 63 of every list is in a lane 63
    uint64_t u[WIDE_KEYS];
    uint64_t tail = WIDE_UPAD, lo = WIDE_UPAD, hi = 0ull, live = 0ull;
#pragma unroll
    for (int j = 0; j < WIDE_KEYS; ++j) {
        const int i = j * WIDE_THREADS + t;
        u[j] = i < n ? wide_u(lists_keys[i]) : WIDE_UPAD;
        if (u[j] != WIDE_UPAD) {
            live += 1ull;
            lo = u[j] < lo ? u[j] : lo;
            hi = u[j] > hi ? u[j] : hi;
        }
        if (lane == MIRROR_KP - 1 && u[j] < tail) tail = u[j];       // a short list's last slot is the pad: it bounds nothing
    }
    auto umin = [](uint64_t a, uint64_t b) { return a < b ? a : b; };
    auto umax = [](uint64_t a, uint64_t b) { return a > b ? a : b; };
    auto usum = [](uint64_t a, uint64_t b) { return a + b; };
    const uint64_t T = wide_reduce(tail, red, umin);
    uint64_t below = 0ull;
#pragma unroll
    for (int j = 0; j < WIDE_KEYS; ++j) below += u[j] < T ? 1ull : 0ull;    // (T == pad: the live keys)
    below = wide_reduce(below, red, usum);

    // (2) the bound. No more than C listed keys below T: K_C >= T. Else K_C < T, by a radix select of rank C among the live keys.
    uint64_t B = T;
    uint32_t source = T == WIDE_UPAD ? WIDE_BOUND_ALL : WIDE_BOUND_TAIL;
    if (below > (uint64_t)c) {
        lo = wide_reduce(lo, red, umin);
        hi = wide_reduce(hi, red, umax);
        int top = 64 - __builtin_clzll(lo ^ hi);         // (more than C >= 1 live keys, all different: lo != hi)
        uint64_t sel = lo;                               // the bits at and above `top` are every live key's
        uint32_t rank = (uint32_t)c;
        while (top > 0) {
            const int w = top < WIDE_DIGIT ? top : WIDE_DIGIT, s = top - w;
            hist[2 * t] = 0u;
            hist[2 * t + 1] = 0u;
            __syncthreads();
            const uint64_t want = wide_above(sel, top);
#pragma unroll
            for (int j = 0; j < WIDE_KEYS; ++j)
                if (u[j] != WIDE_UPAD && wide_above(u[j], top) == want) atomicAdd(&hist[(uint32_t)(u[j] >> s) & ((1u << w) - 1u)], 1u);
            __syncthreads();
            const uint32_t h0 = hist[2 * t], h1 = hist[2 * t + 1], mine = h0 + h1;
            uint32_t incl = mine;
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                const uint32_t v = __shfl_up(incl, o);
                if (lane >= o) incl += v;
            }
            if (lane == WAVE - 1) wave_total[wave] = incl;
            __syncthreads();
            uint32_t excl = incl - mine;
            for (int x = 0; x < wave; ++x) excl += wave_total[x];
            if (rank >= excl && rank < excl + mine) {    // exactly one thread: the keys that match so far number more than `rank`
                const uint32_t odd = rank >= excl + h0 ? 1u : 0u;
                const uint64_t digit = (uint64_t)(2 * t) + odd;
                pick[0] = (top >= 64 ? 0ull : (sel >> top) << top) | (digit << s);
                pick[1] = rank - excl - (odd ? h0 : 0u);
            }
            __syncthreads();
            sel = pick[0];
            rank = (uint32_t)pick[1];
            top = s;
        }
        B = sel;
        source = WIDE_BOUND_RANK;
    }

    // (3) the candidates: the listed keys below B, compacted in any order (at most C by the choice of B), pads behind
    if (t == 0) fill = 0u;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < WIDE_KEYS; ++j) {
        const bool take = u[j] < B;                      // (the pad is below nothing)
        const uint64_t mask = __ballot(take);
        if (mask == 0ull) continue;
        uint32_t base = 0u;
        if (lane == 0) base = atomicAdd(&fill, (uint32_t)__builtin_popcountll(mask));
        base = (uint32_t)__shfl((int)base, 0);
        const uint32_t pos = base + (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
        if (take && pos < (uint32_t)c) cand[pos] = wide_key(u[j]);
    }
    __syncthreads();
    const uint32_t m = fill < (uint32_t)c ? fill : (uint32_t)c;
    for (uint32_t i = m + (uint32_t)t; i < (uint32_t)c; i += WIDE_THREADS) cand[i] = KEY_PAD;
    if (t == 0) {
        ctl[0] = m;
        ctl[1] = source;
        ctl[2] = (uint64_t)wide_key(B);
        ctl[3] = 0ull;
    }
}

// rows of one wave in flight: 4 x 3 float4 per lane at both mirror dimensions, the scan's own depth
constexpr int WIDE_FLIGHT = 4;
template <int DIMS>
struct WideShape {
    static constexpr int GROUP = ScanShape<DIMS>::GROUP, RPW = WAVE / GROUP;
    static constexpr int ROWS_PER_STEP = RPW * SCAN_WAVES, ROWS_PER_BLOCK = ROWS_PER_STEP * WIDE_FLIGHT;
    static_assert(1024 % ROWS_PER_BLOCK == 0 && MIRROR_WIDE_MAX_C % ROWS_PER_BLOCK == 0, "whole workgroups at both C");
};

// (aq stays the first argument: the query is read at its offset in the kernel-argument segment)
template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS) void mirror_wide_rescore_kernel(MirrorWideArgsQ<DIMS> aq) {
    constexpr int D4 = ScanShape<DIMS>::D4, GROUP = ScanShape<DIMS>::GROUP, LOADS = ScanShape<DIMS>::LOADS;
    constexpr int RPW = WideShape<DIMS>::RPW, STEP = WideShape<DIMS>::ROWS_PER_STEP, BLOCK = WideShape<DIMS>::ROWS_PER_BLOCK;
    const MirrorWideArgs& w = aq.w;
    const MirrorScanArgs& a = w.a;
    const int t = (int)threadIdx.x, lane = lane_id(), wave = t >> 6;
    const uint32_t m = (uint32_t)w.ctl[0];
    const uint32_t base = blockIdx.x * (uint32_t)BLOCK;              // (the grid is c / BLOCK: base + BLOCK <= c)
    if (base >= m) {                                                 // a workgroup without a candidate: dead slots
        if (t < BLOCK) w.exact[base + t] = KEY_PAD;
        return;
    }
    const f32x4* q4 = reinterpret_cast<const f32x4*>((const char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(MirrorWideArgsQ<DIMS>, q));
    const int sub = lane / GROUP, gl = lane % GROUP;
    f32x4 q[LOADS];
#pragma unroll
    for (int j = 0; j < LOADS; ++j) q[j] = q4[gl + j * GROUP];
    const f32x4* __restrict__ store4 = reinterpret_cast<const f32x4*>(a.store);
    f32x4 v[WIDE_FLIGHT][LOADS];
    bool live[WIDE_FLIGHT];
    uint32_t grow[WIDE_FLIGHT];
#pragma unroll
    for (int p = 0; p < WIDE_FLIGHT; ++p) {      // every load of the wave in flight before the first product
        const uint32_t i = base + (uint32_t)(p * STEP + wave * RPW + sub);
        const int64_t key = w.cand[i];
        grow[p] = key_row(key);
        const uint32_t lrow = grow[p] - a.row_base;
        live[p] = i < m && key != KEY_PAD && lrow < a.n_rows;
        const f32x4* src = store4 + (size_t)(live[p] ? lrow : 0u) * D4 + gl;
#pragma unroll
        for (int j = 0; j < LOADS; ++j) v[p][j] = src[j * GROUP];
    }
#pragma unroll
    for (int p = 0; p < WIDE_FLIGHT; ++p) {
        const float d = row_distance<GROUP, LOADS, METRIC>(q, v[p], a.q_norm);
        if (gl == GROUP - 1) w.exact[base + (uint32_t)(p * STEP + wave * RPW + sub)] = live[p] ? make_key(d, grow[p]) : KEY_PAD;
    }
}

template <int DIMS, int METRIC, class EPS>
__global__ __launch_bounds__(WIDE_THREADS) void mirror_wide_finish_kernel(MirrorWideArgs w) {
    __shared__ int64_t keys[MIRROR_WIDE_MAX_C];
    const MirrorScanArgs& a = w.a;
    const int t = (int)threadIdx.x;
    const uint32_t m = (uint32_t)w.ctl[0];
    uint32_t n = WAVE;                                   // the sort's size: a power of two >= m, <= c (c is one)
    while (n < m) n <<= 1;
    if (n > (uint32_t)w.c) n = (uint32_t)w.c;
    for (uint32_t i = (uint32_t)t; i < n; i += WIDE_THREADS) keys[i] = i < (uint32_t)w.c ? w.exact[i] : KEY_PAD;
    __syncthreads();
    // bitonic sort, ascending (live keys are unique; the pads end up behind them)
    for (uint32_t span = 2u; span <= n; span <<= 1) {
        for (uint32_t j = span >> 1; j > 0u; j >>= 1) {
            for (uint32_t i = (uint32_t)t; i < n; i += WIDE_THREADS) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const int64_t x = keys[i], y = keys[l];
                    const bool up = (i & span) == 0u;
                    if ((x > y) == up) { keys[i] = y; keys[l] = x; }
                }
            }
            __syncthreads();
        }
    }
    // the k best with frame ids
    for (int i = t; i < a.kpad; i += WIDE_THREADS) {
        wax_hip_hit h;
        h.key = (i < a.k && (uint32_t)i < n) ? keys[i] : KEY_PAD;
        h.frame_id = ID_PAD;
        if (h.key != KEY_PAD) {
            const uint32_t local = key_row(h.key) - a.row_base;
            h.frame_id = (a.ids != nullptr && local < a.n_rows) ? a.ids[local] : (uint64_t)key_row(h.key);
        }
        a.hits[i] = h;
    }
    if (t == 0) {
        const int64_t B = (int64_t)w.ctl[2];
        bool ok = B == KEY_PAD;                          // every listed row is every row, and each was re-scored
        if (!ok && m >= (uint32_t)a.k) {
            const float eps = EPS::template eps<DIMS, METRIC>(a);
            const int64_t kth = keys[a.k - 1];
            const float db = key_distance(B), dk = key_distance(kth);
            ok = kth != KEY_PAD && __builtin_isfinite(db) && __builtin_isfinite(dk) && __builtin_isfinite(eps) && a.q_norm == a.q_norm &&
                 (db - eps > dk);                        // strict: ties stay uncertified
        }
        w.report[0] = w.ctl[0];
        w.report[1] = w.ctl[1];
        w.report[2] = w.ctl[2];
        w.report[3] = 0ull;
        *a.certified = ok ? 1u : 0u;
    }
}

hipError_t launch_mirror_wide_select(const int64_t* d_lists, int lists, int c, int64_t* d_cand, uint64_t* d_ctl, hipStream_t st, int members) {
    if (d_lists == nullptr || d_cand == nullptr || d_ctl == nullptr || lists < 1 || lists > SCAN_KWAY_MERGE_GRID ||
        (c != MIRROR8_DIMS_C && c != 1024 && c != MIRROR_WIDE_MAX_C) || members < 1 || members > MIRROR_MAX_NQ)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mirror_wide_select_kernel, dim3(members), dim3(WIDE_THREADS), 0, st, d_lists, lists, c, d_cand, d_ctl);
    return hipGetLastError();
}

hipError_t launch_mirror_wide(const MirrorWideArgs& w, const float* query, int metric, int bits, hipStream_t st) {
    const MirrorScanArgs& a = w.a;
    if (!mirror_scan_supported(a.dims, metric) || a.n_rows == 0 || a.k < 1 || a.k > MIRROR_WIDE_MAX_K || a.kpad < a.k || a.kpad > MIRROR_WIDE_MAX_K ||
        w.c != mirror_wide_candidates(a.k) || (bits != 8 && bits != 16) || query == nullptr || w.exact == nullptr || w.report == nullptr ||
        a.store == nullptr || a.hits == nullptr || a.certified == nullptr || a.max_bits == nullptr)
        return hipErrorInvalidValue;
    hipError_t err = launch_mirror_wide_select(a.partials, a.lists, w.c, w.cand, w.ctl, st);
    if (err != hipSuccess) return err;
    return with_scan_shape(DimList<384, 768>{}, a.dims, [&](auto s) {
        return with_metric_in<M_COS, M_DOT>(metric, [&](auto mc) {
            constexpr int D = decltype(s)::DIMS, M = decltype(mc)::value;
            MirrorWideArgsQ<D> aq;
            aq.w = w;
            std::memcpy(aq.q, query, sizeof(aq.q));
            hipLaunchKernelGGL((mirror_wide_rescore_kernel<D, M>), dim3(w.c / WideShape<D>::ROWS_PER_BLOCK), dim3(SCAN_THREADS), 0, st, aq);
            hipError_t e2 = hipGetLastError();
            if (e2 != hipSuccess) return e2;
            if (bits == 8) hipLaunchKernelGGL((mirror_wide_finish_kernel<D, M, Mirror8Slack>), dim3(1), dim3(WIDE_THREADS), 0, st, w);
            else hipLaunchKernelGGL((mirror_wide_finish_kernel<D, M, Bf16Eps>), dim3(1), dim3(WIDE_THREADS), 0, st, w);
            return hipGetLastError();
        }, hipErrorInvalidValue);
    }, hipErrorInvalidValue);
}

}  // namespace wax
