// mirror_scan.hip — one query (or up to four) against the bf16 mirror of the store, answered in f32 ("Single queries on
// the mirror").
//
// A single-query scan of a large store is bound by HBM bandwidth alone (scan_kernel: 0.88 of the peak at 10M x 384), so it can only
// get faster by reading fewer bytes. The batched path already keeps a bf16 mirror of the store in step with it (batch_host.inc:
// cosine rows pre-normalised, rows of norm <= 1e-6 zeroed) and a rigorous bound on what its rounding can move a distance by. Two
// launches per pass:
//   the scan    mirror_pass (mirror_pass.h) over Bf16Rows: it streams the mirror (half the f32 bytes); the queries stay f32, mirror
//               values widen exactly (<< 16 / & 0xffff0000). Each workgroup keeps the MIRROR_KP best APPROXIMATE keys of each query.
//                 mirror_scan_kernel          one query, read from the kernel arguments
//                 mirror_scan_masked_kernel   the same under a row bitmap (a predicate search, filter_host.inc): chunks without a
//                                             passing row are not loaded, only passing rows are offered
//                 mirror_scan_group_kernel    2-4 queries ("mirror_share"), read from device memory: one load of a row serves all
//                                             (mirror_group_queries_kernel in front of it copies them there from pinned host memory)
//   the finish  mirror_finish (mirror_finish.h), one workgroup per query: the lists' prefixes under a bound from their heads, sorted
//               (gather_select; the k-way merge of the heads when they overflow its buffer) -> the MIRROR_KP best
//               approximate keys of the store, exact f32 re-score of those rows with scan_kernel's own lane mapping and summation order
//               (bit-identical distances), sort, the k best, frame ids, and the certificate
//                   a_KP - eps > d_k     (a_KP: the KP-th approximate distance, d_k: the exact k-th)
//               Every row outside the candidates has an approximate distance >= a_KP, hence an exact one >= a_KP - eps > d_k: the
//               answer is the f32 scan's. Otherwise the host re-runs the query on the f32 scan (api_search.inc). Under a bitmap the
//               same holds over the passing rows: eps is bounded by maxima over the whole store, the passing rows among them.
#include <cstring>

#include "mirror_finish.h"
#include "mirror_pass.h"

namespace wax {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// The bf16 mirror as a row format of mirror_pass: three dwordx4 (24 bf16) per lane and row, 4 row groups in flight (3 x 4 dwordx4 loads
// per lane, as scan_kernel's 384-d form), no side data, the key an approximate distance.
struct Bf16Rows {
    using Vec = u32x4;
    struct Side {};
    static constexpr int UNROLL = 4;
    static __device__ __forceinline__ Side side(const Side*, uint32_t) { return {}; }
    // two bf16 in dword c -> two f32, exactly (element 2i is the low half)
    static __device__ __forceinline__ f32x2 part(const Vec& v, int c) {
        f32x2 r;
        r.x = __uint_as_float(v[c] << 16);
        r.y = __uint_as_float(v[c] & 0xffff0000u);
        return r;
    }
    static __device__ __forceinline__ float start(const f32x2 (&)[3][4]) { return 0.f; }
    template <int METRIC>
    static __device__ __forceinline__ float key(float s, Side, float inv_qn, float) {
        const float d = METRIC == M_COS ? 1.0f - s * inv_qn : 1.0f - s;
        return (d != d) ? __builtin_inff() : d;
    }
};

}  // namespace

template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS) void mirror_scan_kernel(MirrorScanArgsQ<DIMS> aq) {
    __shared__ int64_t lds[MIRROR_PASS_LDS];
    mirror_pass<Bf16Rows, DIMS, METRIC, 1, false>(reinterpret_cast<const u32x4*>(aq.a.mirror), nullptr, aq.a,
                                                   LoneQuery<MirrorScanArgsQ<DIMS>>{aq.a}, nullptr, lds);
}

// (aq stays the first argument: LoneQuery reads the query at its offset in the kernel-argument segment)
template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS) void mirror_scan_masked_kernel(MirrorScanArgsQ<DIMS> aq, const uint32_t* __restrict__ bitmap) {
    __shared__ int64_t lds[MIRROR_PASS_LDS];
    mirror_pass<Bf16Rows, DIMS, METRIC, 1, true>(reinterpret_cast<const u32x4*>(aq.a.mirror), nullptr, aq.a,
                                                  LoneQuery<MirrorScanArgsQ<DIMS>>{aq.a}, bitmap, lds);
}

template <int DIMS, int METRIC, int NQ>
__global__ __launch_bounds__(SCAN_THREADS) void mirror_scan_group_kernel(MirrorGroupArgs g) {
    static_assert(NQ >= 2, "a lone query has mirror_scan_kernel");
    __shared__ int64_t lds[NQ * MIRROR_PASS_LDS];
    mirror_pass<Bf16Rows, DIMS, METRIC, NQ, false>(reinterpret_cast<const u32x4*>(g.a.mirror), nullptr, g.a, MemberQueries{g.m}, nullptr, lds);
}

template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS) void mirror_finish_kernel(MirrorScanArgsQ<DIMS> aq) {
    mirror_finish<DIMS, METRIC, Bf16Eps>(aq.a, LoneQuery<MirrorScanArgsQ<DIMS>>::kernarg_floats());
}

// one workgroup per member
template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS) void mirror_finish_group_kernel(MirrorGroupArgs g) {
    const MirrorMember& m = g.m[blockIdx.x];
    mirror_finish<DIMS, METRIC, Bf16Eps>(member_args(g.a, m), reinterpret_cast<const f32x4*>(m.query));
}

// the queries of a shared pass from the slots' pinned host buffers into their device buffers, one workgroup per member
__global__ __launch_bounds__(SCAN_THREADS) void mirror_group_queries_kernel(MirrorQueryCopies c) {
    const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(c.src[blockIdx.x]);
    f32x4* __restrict__ dst = reinterpret_cast<f32x4*>(c.dst[blockIdx.x]);
    for (uint32_t i = threadIdx.x; i < c.dims / 4u; i += SCAN_THREADS) dst[i] = src[i];
}

hipError_t launch_mirror_group_queries(const MirrorQueryCopies& c, int nq, hipStream_t st) {
    if (nq < 1 || nq > MIRROR_MAX_NQ || c.dims == 0u || (c.dims & 3u) != 0u) return hipErrorInvalidValue;
    for (int i = 0; i < nq; ++i)
        if (c.src[i] == nullptr || c.dst[i] == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mirror_group_queries_kernel, dim3(nq), dim3(SCAN_THREADS), 0, st, c);
    return hipGetLastError();
}

// mirror_finish's step (1) with mirror_finish's LDS layout and aliasing, then the k-way merge alone (launch_mirror_select_probe)
__global__ __launch_bounds__(SCAN_THREADS) void mirror_select_probe_kernel(const int64_t* __restrict__ lists_keys, int lists, int64_t* __restrict__ out,
                                                                           int* __restrict__ gathered) {
    __shared__ int64_t approx[MIRROR_KP], work[2 * MIRROR_KP], xch[2 * SCAN_WAVES];
    const int t = (int)threadIdx.x;
    bool took;
    if (lists <= SCAN_THREADS) {
        took = gather_select<1>(lists_keys, lists, MIRROR_KP, approx, work, reinterpret_cast<int*>(xch));
        if (!took) kway_merge<1>(lists_keys, lists, MIRROR_KP, approx, xch);
    } else {
        took = gather_select<2>(lists_keys, lists, MIRROR_KP, approx, work, reinterpret_cast<int*>(xch));
        if (!took) kway_merge<2>(lists_keys, lists, MIRROR_KP, approx, xch);
    }
    if (t < MIRROR_KP) out[t] = approx[t];
    if (t == 0) *gathered = took ? 1 : 0;
    __syncthreads();
    if (lists <= SCAN_THREADS) kway_merge<1>(lists_keys, lists, MIRROR_KP, approx, xch);
    else kway_merge<2>(lists_keys, lists, MIRROR_KP, approx, xch);
    if (t < MIRROR_KP) out[MIRROR_KP + t] = approx[t];
}

hipError_t launch_mirror_select_probe(const int64_t* d_lists, int lists, int64_t* d_out, int* d_gathered, hipStream_t st) {
    if (d_lists == nullptr || d_out == nullptr || d_gathered == nullptr || lists < 1 || lists > SCAN_KWAY_MERGE_GRID) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mirror_select_probe_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, d_lists, lists, d_out, d_gathered);
    return hipGetLastError();
}

bool mirror_scan_supported(uint32_t dims, int metric) {
    return in_dim_list(MirrorDims{}, dims) && (metric == M_COS || metric == M_DOT);
}

uint32_t mirror_masked_chunk_rows(uint32_t dims) {
    return with_scan_shape(MirrorDims{}, dims, [](auto s) { return (uint32_t)MirrorShape<Bf16Rows, decltype(s)::DIMS>::RPC; }, 0u);
}

namespace {
// the lone query's two launches, with or without a bitmap
hipError_t launch_lone(const MirrorScanArgs& args, const uint32_t* bitmap, const float* query, int metric, int grid_cap, hipStream_t st) {
    return with_mirror_pass<Bf16Rows>(args.n_rows, args.dims, metric, grid_cap, [&](auto s, auto m, int grid) {
        constexpr int D = decltype(s)::DIMS, M = decltype(m)::value;
        MirrorScanArgsQ<D> aq;
        aq.a = args;
        aq.a.lists = grid;
        std::memcpy(aq.q, query, sizeof(aq.q));
        if (bitmap != nullptr) launch_kernel((mirror_scan_masked_kernel<D, M>), dim3(grid), dim3(SCAN_THREADS), 0, st, aq, bitmap);
        else launch_kernel((mirror_scan_kernel<D, M>), dim3(grid), dim3(SCAN_THREADS), 0, st, aq);
        return launch_finish((mirror_finish_kernel<D, M>), 1, st, aq);
    });
}
}  // namespace

hipError_t launch_mirror_scan(const MirrorScanArgs& args, const float* query, int metric, int grid_cap, hipStream_t st) {
    if (!mirror_launch_ok(args, metric, MIRROR_MAX_K)) return hipErrorInvalidValue;
    return launch_lone(args, nullptr, query, metric, grid_cap, st);
}

hipError_t launch_mirror_scan_masked(const MirrorScanArgs& args, const uint32_t* bitmap, const float* query, int metric, int grid_cap, hipStream_t st) {
    if (!mirror_launch_ok(args, metric, MIRROR_MAX_K) || bitmap == nullptr) return hipErrorInvalidValue;
    return launch_lone(args, bitmap, query, metric, grid_cap, st);
}

hipError_t launch_mirror_group(const MirrorGroupArgs& args, int nq, int metric, int grid_cap, hipStream_t st) {
    if (!mirror_launch_ok(args.a, metric, MIRROR_MAX_K, args.m, nq)) return hipErrorInvalidValue;
    return with_mirror_pass<Bf16Rows>(args.a.n_rows, args.a.dims, metric, grid_cap, [&](auto s, auto m, int grid) {
        constexpr int D = decltype(s)::DIMS, M = decltype(m)::value;
        MirrorGroupArgs g = args;
        g.a.lists = grid;
        return with_group_size(nq, [&](auto c) {
            launch_kernel((mirror_scan_group_kernel<D, M, decltype(c)::value>), dim3(grid), dim3(SCAN_THREADS), 0, st, g);
            return launch_finish((mirror_finish_group_kernel<D, M>), nq, st, g);
        });
    });
}

}  // namespace wax
