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

template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS) void mirror_finish_kernel(MirrorScanArgsQ<DIMS> aq) {
    constexpr int D4 = ScanShape<DIMS>::D4;
    constexpr int GROUP = ScanShape<DIMS>::GROUP;
    constexpr int LOADS = ScanShape<DIMS>::LOADS;
    constexpr int RPW = WAVE / GROUP;
    constexpr int ROWS_PER_PASS = RPW * SCAN_WAVES;
    constexpr int PASSES = MIRROR_KP / ROWS_PER_PASS;
    static_assert(MIRROR_KP % ROWS_PER_PASS == 0, "whole passes");
    const MirrorScanArgs& a = aq.a;
    __shared__ int64_t approx[MIRROR_KP], exact[MIRROR_KP], sorted[MIRROR_KP], xch[2 * SCAN_WAVES];
    const int t = (int)threadIdx.x;
    const int lane = lane_id();
    const int wave = t >> 6;

    // (1) the MIRROR_KP best approximate keys of the whole store
    if (a.lists <= SCAN_THREADS) kway_merge<1>(a.partials, a.lists, MIRROR_KP, approx, xch);
    else kway_merge<2>(a.partials, a.lists, MIRROR_KP, approx, xch);

    // (2) exact f32 re-score of those rows: row_distance (row_math.h) at the f32 scan's shape for this dimension
    const char* ka = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
    const f32x4* q4 = reinterpret_cast<const f32x4*>(ka + offsetof(MirrorScanArgsQ<DIMS>, q));
    const int sub = lane / GROUP, gl = lane % GROUP;
    f32x4 q[LOADS];
#pragma unroll
    for (int j = 0; j < LOADS; ++j) q[j] = q4[gl + j * GROUP];
    const f32x4* __restrict__ store4 = reinterpret_cast<const f32x4*>(a.store);
    f32x4 v[PASSES][LOADS];
    bool live[PASSES];
    uint32_t grow[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {   // every load of the wave in flight before the first product
        const int i = p * ROWS_PER_PASS + wave * RPW + sub;
        const int64_t key = approx[i];
        grow[p] = key_row(key);
        const uint32_t lrow = grow[p] - a.row_base;
        live[p] = key != KEY_PAD && lrow < a.n_rows;
        const f32x4* src = store4 + (size_t)(live[p] ? lrow : 0u) * D4 + gl;
#pragma unroll
        for (int j = 0; j < LOADS; ++j) v[p][j] = src[j * GROUP];
    }
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const float d = row_distance<GROUP, LOADS, METRIC>(q, v[p], a.q_norm);
        if (gl == GROUP - 1) exact[p * ROWS_PER_PASS + wave * RPW + sub] = live[p] ? make_key(d, grow[p]) : KEY_PAD;
    }
    __syncthreads();

    // (3) rank sort of the exact keys (unique rows; KEY_PAD ties broken by position)
    if (t < MIRROR_KP) {
        const int64_t key = exact[t];
        int rank = 0;
        for (int j = 0; j < MIRROR_KP; ++j) {
            const int64_t o = exact[j];
            rank += (o < key || (o == key && j < t)) ? 1 : 0;
        }
        sorted[rank] = key;
    }
    __syncthreads();

    // (4) the k best with frame ids; (5) the certificate
    for (int i = t; i < a.kpad; i += SCAN_THREADS) {
        wax_hip_hit h;
        h.key = (i < a.k) ? sorted[i] : KEY_PAD;
        h.frame_id = ID_PAD;
        if (h.key != KEY_PAD) {
            const uint32_t local = key_row(h.key) - a.row_base;
            h.frame_id = (a.ids != nullptr && local < a.n_rows) ? a.ids[local] : (uint64_t)key_row(h.key);
        }
        a.hits[i] = h;
    }
    if (t == 0) {
        // eps: batch_prep_kernel's bound (batch.hip) with the query-side rounding term gone — the query is not rounded. With x_v the
        // f32 row that was rounded (normalised for cosine) and v~ its bf16 rounding, |q.v~ - q.x_v| <= ||q|| ||v~ - x_v||, bounded by
        // ||q|| max_rows ||v~ - x_v|| (measured when the mirror was converted, + 0.1 % for its f32 accumulation); the f32 sums on
        // either side and the normalisations stay inside 3 D 2^-24 of ||q|| max||v||; the exact distance carries ~1e-6 of its own.
        // Without a measurement: the worst case of one rounded operand is below the batched path's two-operand constant, kept as is.
        // Cosine divides by ||q||, so both norms are 1 there.
        const unsigned int* mb = a.max_bits;
        const float max_norm = __uint_as_float(mb[0]);
        const float max_row_err = a.use_measured ? __uint_as_float(mb[1]) : 0.f;
        const double qn_d = METRIC == M_COS ? 1.0 + 1e-6 : (double)a.q_norm;
        const double vn_d = METRIC == M_COS ? 1.0 + 1e-6 : (double)max_norm;
        const double u = 0.0078125 * (1.0 + 1.0 / 512.0) + (double)DIMS * 5.97e-8 + 1e-6;
        double dot_err = u * qn_d * vn_d * 1.001;
        if (max_row_err > 0.f) {
            const double measured = qn_d * (double)max_row_err * 1.001 + 3.0 * (double)DIMS * 5.97e-8 * qn_d * vn_d;
            if (measured < dot_err) dot_err = measured;
        }
        float eps = METRIC == M_COS ? (float)(dot_err + 3e-6) : (float)(dot_err + 1e-6 * (1.0 + qn_d * vn_d));
        eps = nextafterf(eps, __builtin_inff());             // the double -> float conversion may have rounded down
        const int64_t a_kp = approx[MIRROR_KP - 1], kth = sorted[a.k - 1];
        const float da = key_distance(a_kp), dk = key_distance(kth);
        const bool ok = a_kp != KEY_PAD && kth != KEY_PAD && __builtin_isfinite(da) && __builtin_isfinite(dk) &&
                        __builtin_isfinite(eps) && a.q_norm == a.q_norm && (da - eps > dk);   // strict: ties stay uncertified
        *a.certified = ok ? 1u : 0u;
    }
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

}  // namespace wax
