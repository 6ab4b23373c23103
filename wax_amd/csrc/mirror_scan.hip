// mirror_scan.hip — one query against the bf16 mirror of the store, answered in f32 ("Single queries on the mirror").
//
// A single-query scan of a large store is bound by HBM bandwidth alone (scan_kernel: 0.88 of the peak at 10M x 384), so it can only
// get faster by reading fewer bytes. The batched path already keeps a bf16 mirror of the store in step with it (batch_host.inc:
// cosine rows pre-normalised, rows of norm <= 1e-6 zeroed) and a rigorous bound on what its rounding can move a distance by. Two
// launches per query:
//   mirror_scan_kernel    streams the mirror (half the f32 bytes) with scan_kernel's structure: persistent grid, GROUP lanes per row,
//                         non-temporal dwordx4 loads, UNROLL row groups in flight, DPP group sums, the per-wave top-k lists and the
//                         workgroup rank merge. The query stays f32 (kernel arguments, VGPRs); mirror values widen exactly
//                         (<< 16 / & 0xffff0000). Each workgroup keeps the MIRROR_KP best APPROXIMATE keys.
//   mirror_finish_kernel  one workgroup: k-way merge of the lists' heads -> the MIRROR_KP best approximate keys of the store, exact f32
//                         re-score of those rows with scan_kernel's own lane mapping and summation order (bit-identical distances),
//                         sort, the k best, frame ids, and the certificate
//                             a_KP - eps > d_k     (a_KP: the KP-th approximate distance, d_k: the exact k-th)
//                         Every row outside the candidates has an approximate distance >= a_KP, hence an exact one >= a_KP - eps > d_k:
//                         the answer is the f32 scan's. Otherwise the host re-runs the query on the f32 scan (api_search.inc).
//   mirror_scan_masked_kernel  the first launch under a row bitmap (a predicate search, filter_host.inc): chunks without a passing row
//                         are not loaded, only passing rows are offered; the same finish, the same certificate over the passing rows.
#include <cstddef>
#include <cstring>

#include "kernels.h"
#include "row_math.h"
#include "topk.h"

namespace wax {

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int MIRROR_UNROLL = 4;      // row groups in flight per wave: 3 x 4 dwordx4 loads per lane, as scan_kernel's 384-d form

// two bf16 in one dword -> two f32, exactly (element 2i is the low half)
__device__ inline f32x2 widen(unsigned int w) {
    f32x2 r;
    r.x = __uint_as_float(w << 16);
    r.y = __uint_as_float(w & 0xffff0000u);
    return r;
}

// The dimensions with a mirror scan: the BASELINE pair (three dwordx4 of bf16 per lane and row divide them; kernel arguments hold
// the query). The exact re-score takes its lanes per row from ScanShape<DIMS> (row_math.h), like every exact path.
using MirrorDims = DimList<384, 768>;

// mirror lanes per row: three dwordx4 (24 bf16) per lane and row
template <int DIMS> struct MirrorShape { static constexpr int D8 = DIMS / 8, GROUP = D8 / 3; };

}  // namespace

template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS) void mirror_scan_kernel(MirrorScanArgsQ<DIMS> aq) {
    constexpr int D8 = MirrorShape<DIMS>::D8;      // dwordx4 (8 bf16) per row
    constexpr int GROUP = MirrorShape<DIMS>::GROUP;
    constexpr int LOADS = D8 / GROUP;
    constexpr int RPW = WAVE / GROUP;
    constexpr int RPC = RPW * MIRROR_UNROLL;
    constexpr int CAP = 128;
    static_assert(LOADS == 3 && D8 % GROUP == 0, "three dwordx4 per lane and row");
    const MirrorScanArgs& a = aq.a;
    __shared__ int64_t lds[SCAN_WAVES * CAP + SCAN_WAVES + MIRROR_KP];

    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const int sub = lane / GROUP;
    const int gl = lane % GROUP;
    const bool owner = (gl == GROUP - 1);
    const uint32_t n = a.n_rows;

    // the query slice of this lane: elements [8c, 8c + 8) of chunk c = gl + j * GROUP, straight from the kernel arguments
    const char* ka = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
    const f32x4* q4 = reinterpret_cast<const f32x4*>(ka + offsetof(MirrorScanArgsQ<DIMS>, q));
    f32x2 q[LOADS][4];
#pragma unroll
    for (int j = 0; j < LOADS; ++j) {
        const f32x4 lo = q4[2 * (gl + j * GROUP)], hi = q4[2 * (gl + j * GROUP) + 1];
        q[j][0] = lo.xy; q[j][1] = lo.zw; q[j][2] = hi.xy; q[j][3] = hi.zw;
    }
    // cosine: mirror rows are unit vectors (or zero), so sim = acc / ||q||; the rule for a null query is the f32 scan's
    const float inv_qn = a.q_norm > COS_NORM_FLOOR ? 1.0f / a.q_norm : 0.0f;

    const u32x4* __restrict__ mirror4 = reinterpret_cast<const u32x4*>(a.mirror);
    WaveTopK<CAP> tk;
    tk.init(lds + wave * CAP, MIRROR_KP);

    const uint32_t nchunks = (n + RPC - 1) / RPC;
    const uint32_t gwave = blockIdx.x * SCAN_WAVES + wave;
    const uint32_t nwaves = gridDim.x * SCAN_WAVES;

    for (uint32_t chunk = gwave; chunk < nchunks; chunk += nwaves) {
        const uint32_t rbase = chunk * RPC + sub;
        tk.make_room(RPC);
        u32x4 v[MIRROR_UNROLL][LOADS];
#pragma unroll
        for (int u = 0; u < MIRROR_UNROLL; ++u) {
            const uint32_t r = rbase + u * RPW;
            const uint32_t rc = r < n ? r : n - 1;  // clamp: tail lanes re-read the last row, result discarded
            const u32x4* p = mirror4 + (size_t)rc * D8 + gl;
#pragma unroll
            for (int j = 0; j < LOADS; ++j) v[u][j] = __builtin_nontemporal_load(p + j * GROUP);
        }
#pragma unroll
        for (int u = 0; u < MIRROR_UNROLL; ++u) {
            f32x2 acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
            for (int j = 0; j < LOADS; ++j) {
                acc[0] = __builtin_elementwise_fma(q[j][0], widen(v[u][j].x), acc[0]);
                acc[1] = __builtin_elementwise_fma(q[j][1], widen(v[u][j].y), acc[1]);
                acc[2] = __builtin_elementwise_fma(q[j][2], widen(v[u][j].z), acc[2]);
                acc[3] = __builtin_elementwise_fma(q[j][3], widen(v[u][j].w), acc[3]);
            }
            const f32x2 s2 = (acc[0] + acc[1]) + (acc[2] + acc[3]);
            const float s = group_sum<GROUP>(s2.x + s2.y);
            float d = METRIC == M_COS ? 1.0f - s * inv_qn : 1.0f - s;
            d = (d != d) ? __builtin_inff() : d;
            const uint32_t r = rbase + u * RPW;
            tk.push(make_key(d + 0.0f, a.row_base + r), owner && (r < n));
        }
    }

    int* counts = reinterpret_cast<int*>(lds + SCAN_WAVES * CAP);
    int64_t* fin = lds + SCAN_WAVES * CAP + SCAN_WAVES;
    tk.finalize();
    if (lane == 0) counts[wave] = tk.cnt;
    __syncthreads();
    block_rank_merge<SCAN_WAVES>(lds, CAP, counts, MIRROR_KP, fin);
    __syncthreads();
    int64_t* mine = a.partials + (size_t)blockIdx.x * MIRROR_KP;
    for (int t = (int)threadIdx.x; t < MIRROR_KP; t += SCAN_THREADS) mine[t] = fin[t];
}

// ---- under a row bitmap (wax_hip_search_predicate) ---------------------------------------------------------------------
// mirror_scan_kernel with the row bitmap of predicate.hip, in scan_masked_kernel's form: the wave's chunk of RPC rows is the unit of
// the skip test; its bits are requested one iteration ahead and made wave-uniform; a chunk without a passing row is not loaded; a row
// is offered only when its bit is set. Everything between the loads and the key is the unmasked kernel's text, so a passing row's
// approximate key is the one it gets without a mask, and the workgroup's list holds the MIRROR_KP best approximate keys among ITS
// passing rows. The finish is mirror_finish_kernel as it is: eps is bounded by maxima over the whole store, the passing rows among them.
template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS) void mirror_scan_masked_kernel(MirrorScanArgsQ<DIMS> aq, const uint32_t* __restrict__ bitmap) {
    constexpr int D8 = MirrorShape<DIMS>::D8;
    constexpr int GROUP = MirrorShape<DIMS>::GROUP;
    constexpr int LOADS = D8 / GROUP;
    constexpr int RPW = WAVE / GROUP;
    constexpr int RPC = RPW * MIRROR_UNROLL;
    constexpr int CAP = 128;
    static_assert(LOADS == 3 && D8 % GROUP == 0, "three dwordx4 per lane and row");
    static_assert((RPC & (RPC - 1)) == 0 && RPC <= 32, "a chunk's bits must sit inside one bitmap word");
    const MirrorScanArgs& a = aq.a;
    __shared__ int64_t lds[SCAN_WAVES * CAP + SCAN_WAVES + MIRROR_KP];

    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const int sub = lane / GROUP;
    const int gl = lane % GROUP;
    const bool owner = (gl == GROUP - 1);
    const uint32_t n = a.n_rows;

    // the query slice of this lane, straight from the kernel arguments (aq is the first argument: its offsets are the segment's)
    const char* ka = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
    const f32x4* q4 = reinterpret_cast<const f32x4*>(ka + offsetof(MirrorScanArgsQ<DIMS>, q));
    f32x2 q[LOADS][4];
#pragma unroll
    for (int j = 0; j < LOADS; ++j) {
        const f32x4 lo = q4[2 * (gl + j * GROUP)], hi = q4[2 * (gl + j * GROUP) + 1];
        q[j][0] = lo.xy; q[j][1] = lo.zw; q[j][2] = hi.xy; q[j][3] = hi.zw;
    }
    const float inv_qn = a.q_norm > COS_NORM_FLOOR ? 1.0f / a.q_norm : 0.0f;

    const u32x4* __restrict__ mirror4 = reinterpret_cast<const u32x4*>(a.mirror);
    WaveTopK<CAP> tk;
    tk.init(lds + wave * CAP, MIRROR_KP);

    const uint32_t nchunks = (n + RPC - 1) / RPC;
    const uint32_t gwave = blockIdx.x * SCAN_WAVES + wave;
    const uint32_t nwaves = gridDim.x * SCAN_WAVES;

    // (one iteration ahead: predicate.hip, scan_masked_kernel)
    uint32_t word = gwave < nchunks ? bitmap[(gwave * RPC) >> 5] : 0u;
    for (uint32_t chunk = gwave; chunk < nchunks; chunk += nwaves) {
        const uint32_t r0 = chunk * RPC;                     // < n: word r0 >> 5 exists; bits of rows >= n are clear
        const uint32_t bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)((word >> (r0 & 31u)) & (uint32_t)((1ull << RPC) - 1ull)));
        const uint32_t next = chunk + nwaves;
        if (next < nchunks) word = bitmap[(next * RPC) >> 5];
        if (bits == 0u) continue;                            // wave-uniform: no row of the chunk may be offered, so none is loaded
        const uint32_t rbase = r0 + sub;
        tk.make_room(RPC);
        u32x4 v[MIRROR_UNROLL][LOADS];
#pragma unroll
        for (int u = 0; u < MIRROR_UNROLL; ++u) {
            const uint32_t r = rbase + u * RPW;
            const uint32_t rc = r < n ? r : n - 1;  // clamp: tail lanes re-read the last row, result discarded
            const u32x4* p = mirror4 + (size_t)rc * D8 + gl;
#pragma unroll
            for (int j = 0; j < LOADS; ++j) v[u][j] = __builtin_nontemporal_load(p + j * GROUP);
        }
#pragma unroll
        for (int u = 0; u < MIRROR_UNROLL; ++u) {
            f32x2 acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
            for (int j = 0; j < LOADS; ++j) {
                acc[0] = __builtin_elementwise_fma(q[j][0], widen(v[u][j].x), acc[0]);
                acc[1] = __builtin_elementwise_fma(q[j][1], widen(v[u][j].y), acc[1]);
                acc[2] = __builtin_elementwise_fma(q[j][2], widen(v[u][j].z), acc[2]);
                acc[3] = __builtin_elementwise_fma(q[j][3], widen(v[u][j].w), acc[3]);
            }
            const f32x2 s2 = (acc[0] + acc[1]) + (acc[2] + acc[3]);
            const float s = group_sum<GROUP>(s2.x + s2.y);
            float d = METRIC == M_COS ? 1.0f - s * inv_qn : 1.0f - s;
            d = (d != d) ? __builtin_inff() : d;
            const uint32_t r = rbase + u * RPW;
            const bool bit = ((bits >> (uint32_t)(sub + u * RPW)) & 1u) != 0u;
            tk.push(make_key(d + 0.0f, a.row_base + r), owner && (r < n) && bit);
        }
    }

    int* counts = reinterpret_cast<int*>(lds + SCAN_WAVES * CAP);
    int64_t* fin = lds + SCAN_WAVES * CAP + SCAN_WAVES;
    tk.finalize();
    if (lane == 0) counts[wave] = tk.cnt;
    __syncthreads();
    block_rank_merge<SCAN_WAVES>(lds, CAP, counts, MIRROR_KP, fin);
    __syncthreads();
    int64_t* mine = a.partials + (size_t)blockIdx.x * MIRROR_KP;
    for (int t = (int)threadIdx.x; t < MIRROR_KP; t += SCAN_THREADS) mine[t] = fin[t];
}

template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS) void mirror_finish_kernel(MirrorScanArgsQ<DIMS> aq) {
    const MirrorScanArgs& a = aq.a;
#define MIRROR_FINISH_QUERY reinterpret_cast<const f32x4*>((const char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(MirrorScanArgsQ<DIMS>, q))
#include "mirror_finish_body.inc"
#undef MIRROR_FINISH_QUERY
}

// ---- several queries per pass ----------------------------------------------------------------------------------------------------
// mirror_scan_kernel with NQ accumulator sets: the row loads, the clamp and the widening are shared, everything from the first fma to
// the workgroup's list is per query and is the single-query kernel's code (four f32x2 chains, the (acc0+acc1)+(acc2+acc3) tree,
// group_sum, 1 - s * inv_qn), so a member's approximate keys are the ones it would get alone.
template <int DIMS, int METRIC, int NQ>
__global__ __launch_bounds__(SCAN_THREADS) void mirror_scan_group_kernel(MirrorGroupArgs g) {
    constexpr int D8 = MirrorShape<DIMS>::D8;
    constexpr int GROUP = MirrorShape<DIMS>::GROUP;
    constexpr int LOADS = D8 / GROUP;
    constexpr int RPW = WAVE / GROUP;
    constexpr int RPC = RPW * MIRROR_UNROLL;
    constexpr int CAP = 128;
    constexpr int PER_Q = SCAN_WAVES * CAP + SCAN_WAVES + MIRROR_KP;
    static_assert(LOADS == 3 && D8 % GROUP == 0, "three dwordx4 per lane and row");
    static_assert(NQ >= 2 && NQ <= MIRROR_MAX_NQ, "queries per pass");
    const MirrorScanArgs& a = g.a;
    __shared__ int64_t lds[NQ * PER_Q];

    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const int sub = lane / GROUP;
    const int gl = lane % GROUP;
    const bool owner = (gl == GROUP - 1);
    const uint32_t n = a.n_rows;

    f32x2 q[NQ][LOADS][4];
    float inv_qn[NQ];
    WaveTopK<CAP> tk[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const f32x4* q4 = reinterpret_cast<const f32x4*>(g.m[i].query);
#pragma unroll
        for (int j = 0; j < LOADS; ++j) {
            const f32x4 lo = q4[2 * (gl + j * GROUP)], hi = q4[2 * (gl + j * GROUP) + 1];
            q[i][j][0] = lo.xy; q[i][j][1] = lo.zw; q[i][j][2] = hi.xy; q[i][j][3] = hi.zw;
        }
        inv_qn[i] = g.m[i].q_norm > COS_NORM_FLOOR ? 1.0f / g.m[i].q_norm : 0.0f;
        tk[i].init(lds + i * PER_Q + wave * CAP, MIRROR_KP);
    }

    const u32x4* __restrict__ mirror4 = reinterpret_cast<const u32x4*>(a.mirror);
    const uint32_t nchunks = (n + RPC - 1) / RPC;
    const uint32_t gwave = blockIdx.x * SCAN_WAVES + wave;
    const uint32_t nwaves = gridDim.x * SCAN_WAVES;

    for (uint32_t chunk = gwave; chunk < nchunks; chunk += nwaves) {
        const uint32_t rbase = chunk * RPC + sub;
#pragma unroll
        for (int i = 0; i < NQ; ++i) tk[i].make_room(RPC);
        u32x4 v[MIRROR_UNROLL][LOADS];
#pragma unroll
        for (int u = 0; u < MIRROR_UNROLL; ++u) {
            const uint32_t r = rbase + u * RPW;
            const uint32_t rc = r < n ? r : n - 1;  // clamp: tail lanes re-read the last row, result discarded
            const u32x4* p = mirror4 + (size_t)rc * D8 + gl;
#pragma unroll
            for (int j = 0; j < LOADS; ++j) v[u][j] = __builtin_nontemporal_load(p + j * GROUP);
        }
#pragma unroll
        for (int u = 0; u < MIRROR_UNROLL; ++u) {
            f32x2 w[LOADS][4];              // widened once, used by every query
#pragma unroll
            for (int j = 0; j < LOADS; ++j) {
                w[j][0] = widen(v[u][j].x); w[j][1] = widen(v[u][j].y); w[j][2] = widen(v[u][j].z); w[j][3] = widen(v[u][j].w);
            }
            const uint32_t r = rbase + u * RPW;
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                f32x2 acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
                for (int j = 0; j < LOADS; ++j) {
                    acc[0] = __builtin_elementwise_fma(q[i][j][0], w[j][0], acc[0]);
                    acc[1] = __builtin_elementwise_fma(q[i][j][1], w[j][1], acc[1]);
                    acc[2] = __builtin_elementwise_fma(q[i][j][2], w[j][2], acc[2]);
                    acc[3] = __builtin_elementwise_fma(q[i][j][3], w[j][3], acc[3]);
                }
                const f32x2 s2 = (acc[0] + acc[1]) + (acc[2] + acc[3]);
                const float s = group_sum<GROUP>(s2.x + s2.y);
                float d = METRIC == M_COS ? 1.0f - s * inv_qn[i] : 1.0f - s;
                d = (d != d) ? __builtin_inff() : d;
                tk[i].push(make_key(d + 0.0f, a.row_base + r), owner && (r < n));
            }
        }
    }

#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        tk[i].finalize();
        int* counts = reinterpret_cast<int*>(lds + i * PER_Q + SCAN_WAVES * CAP);
        if (lane == 0) counts[wave] = tk[i].cnt;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        int64_t* base = lds + i * PER_Q;
        block_rank_merge<SCAN_WAVES>(base, CAP, reinterpret_cast<int*>(base + SCAN_WAVES * CAP), MIRROR_KP, base + SCAN_WAVES * CAP + SCAN_WAVES);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int64_t* fin = lds + i * PER_Q + SCAN_WAVES * CAP + SCAN_WAVES;
        int64_t* mine = g.m[i].partials + (size_t)blockIdx.x * MIRROR_KP;
        for (int t = (int)threadIdx.x; t < MIRROR_KP; t += SCAN_THREADS) mine[t] = fin[t];
    }
}

// one workgroup per member: the single-query finish with the member's own lists, hits, certificate word, norm and k
template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS) void mirror_finish_group_kernel(MirrorGroupArgs g) {
    const MirrorMember& m = g.m[blockIdx.x];
    MirrorScanArgs a = g.a;
    a.partials = m.partials;
    a.hits = m.hits;
    a.certified = m.certified;
    a.q_norm = m.q_norm;
    a.k = m.k;
    a.kpad = m.kpad;
#define MIRROR_FINISH_QUERY reinterpret_cast<const f32x4*>(m.query)
#include "mirror_finish_body.inc"
#undef MIRROR_FINISH_QUERY
}

namespace {
template <int DIMS, int METRIC>
hipError_t launch_mirror_dims(const MirrorScanArgs& args, const float* query, int grid, hipStream_t st) {
    MirrorScanArgsQ<DIMS> aq;
    aq.a = args;
    aq.a.lists = grid;
    std::memcpy(aq.q, query, sizeof(aq.q));
    launch_kernel((mirror_scan_kernel<DIMS, METRIC>), dim3(grid), dim3(SCAN_THREADS), 0, st, aq);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL((mirror_finish_kernel<DIMS, METRIC>), dim3(1), dim3(SCAN_THREADS), 0, st, aq);
    return hipGetLastError();
}
template <int DIMS, int METRIC>
hipError_t launch_mirror_masked_dims(const MirrorScanArgs& args, const uint32_t* bitmap, const float* query, int grid, hipStream_t st) {
    MirrorScanArgsQ<DIMS> aq;
    aq.a = args;
    aq.a.lists = grid;
    std::memcpy(aq.q, query, sizeof(aq.q));
    launch_kernel((mirror_scan_masked_kernel<DIMS, METRIC>), dim3(grid), dim3(SCAN_THREADS), 0, st, aq, bitmap);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL((mirror_finish_kernel<DIMS, METRIC>), dim3(1), dim3(SCAN_THREADS), 0, st, aq);
    return hipGetLastError();
}
template <int DIMS, int METRIC>
hipError_t launch_group_dims(const MirrorGroupArgs& args, int nq, int grid, hipStream_t st) {
    MirrorGroupArgs g = args;
    g.a.lists = grid;
    switch (nq) {
        case 2: launch_kernel((mirror_scan_group_kernel<DIMS, METRIC, 2>), dim3(grid), dim3(SCAN_THREADS), 0, st, g); break;
        case 3: launch_kernel((mirror_scan_group_kernel<DIMS, METRIC, 3>), dim3(grid), dim3(SCAN_THREADS), 0, st, g); break;
        case 4: launch_kernel((mirror_scan_group_kernel<DIMS, METRIC, 4>), dim3(grid), dim3(SCAN_THREADS), 0, st, g); break;
        default: return hipErrorInvalidValue;
    }
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL((mirror_finish_group_kernel<DIMS, METRIC>), dim3(nq), dim3(SCAN_THREADS), 0, st, g);
    return hipGetLastError();
}
}  // namespace

bool mirror_scan_supported(uint32_t dims, int metric) {
    return in_dim_list(MirrorDims{}, dims) && (metric == M_COS || metric == M_DOT);
}

int mirror_grid_for(uint32_t n_rows, uint32_t dims, int grid_cap) {
    // scan_grid_for's large-store rule with the mirror kernel's rows per wave iteration: at most grid_cap (default 512 = 2 per CU)
    // workgroups, every wave the same number of iterations (+-1 chunk in total)
    if (grid_cap <= 0) grid_cap = 512;
    if (grid_cap > SCAN_KWAY_MERGE_GRID) grid_cap = SCAN_KWAY_MERGE_GRID;
    const uint64_t rpc = (uint64_t)(WAVE / (dims / 24)) * MIRROR_UNROLL;
    const uint64_t nchunks = ((uint64_t)n_rows + rpc - 1) / rpc;
    const uint64_t max_waves = (uint64_t)grid_cap * SCAN_WAVES;
    uint64_t waves = nchunks;
    if (nchunks > max_waves) {
        const uint64_t iters = (nchunks + max_waves - 1) / max_waves;
        waves = (nchunks + iters - 1) / iters;
    }
    uint64_t blocks = (waves + SCAN_WAVES - 1) / SCAN_WAVES;
    if (blocks < 1) blocks = 1;
    if (blocks > (uint64_t)grid_cap) blocks = grid_cap;
    return (int)blocks;
}

hipError_t launch_mirror_scan(const MirrorScanArgs& args, const float* query, int metric, int grid_cap, hipStream_t st) {
    if (!mirror_scan_supported(args.dims, metric) || args.k < 1 || args.k > MIRROR_MAX_K || args.kpad < args.k || args.n_rows == 0)
        return hipErrorInvalidValue;
    const int grid = mirror_grid_for(args.n_rows, args.dims, grid_cap);
    return with_scan_shape(MirrorDims{}, args.dims, [&](auto s) {
        return with_metric_in<M_COS, M_DOT>(metric, [&](auto m) {
            return launch_mirror_dims<decltype(s)::DIMS, decltype(m)::value>(args, query, grid, st);
        }, hipErrorInvalidValue);
    }, hipErrorInvalidValue);
}

uint32_t mirror_masked_chunk_rows(uint32_t dims) {
    return in_dim_list(MirrorDims{}, dims) ? (uint32_t)(WAVE / (dims / 24)) * MIRROR_UNROLL : 0u;   // RPC of mirror_scan_masked_kernel
}

hipError_t launch_mirror_scan_masked(const MirrorScanArgs& args, const uint32_t* bitmap, const float* query, int metric, int grid_cap, hipStream_t st) {
    if (!mirror_scan_supported(args.dims, metric) || args.k < 1 || args.k > MIRROR_MAX_K || args.kpad < args.k || args.n_rows == 0 || bitmap == nullptr)
        return hipErrorInvalidValue;
    const int grid = mirror_grid_for(args.n_rows, args.dims, grid_cap);
    return with_scan_shape(MirrorDims{}, args.dims, [&](auto s) {
        return with_metric_in<M_COS, M_DOT>(metric, [&](auto m) {
            return launch_mirror_masked_dims<decltype(s)::DIMS, decltype(m)::value>(args, bitmap, query, grid, st);
        }, hipErrorInvalidValue);
    }, hipErrorInvalidValue);
}

hipError_t launch_mirror_group(const MirrorGroupArgs& args, int nq, int metric, int grid_cap, hipStream_t st) {
    if (!mirror_scan_supported(args.a.dims, metric) || nq < 2 || nq > MIRROR_MAX_NQ || args.a.n_rows == 0) return hipErrorInvalidValue;
    for (int i = 0; i < nq; ++i)
        if (args.m[i].k < 1 || args.m[i].k > MIRROR_MAX_K || args.m[i].kpad < args.m[i].k || args.m[i].query == nullptr) return hipErrorInvalidValue;
    const int grid = mirror_grid_for(args.a.n_rows, args.a.dims, grid_cap);
    return with_scan_shape(MirrorDims{}, args.a.dims, [&](auto s) {
        return with_metric_in<M_COS, M_DOT>(metric, [&](auto m) {
            return launch_group_dims<decltype(s)::DIMS, decltype(m)::value>(args, nq, grid, st);
        }, hipErrorInvalidValue);
    }, hipErrorInvalidValue);
}

}  // namespace wax
