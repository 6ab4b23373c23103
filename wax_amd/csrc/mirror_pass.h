// mirror_pass.h — ONE pass of NQ queries over a compressed mirror of the store, optionally under a row bitmap: the scan body of every
// kernel of mirror_scan.hip, and the host side of every pass, mirror8_scan.hip's included. The 8-bit pass has a
// body of its own on the matrix pipe (code8_pass, mirror8_scan.hip) inside the same frame: queries, grid rule, lists, partials.
//
// scan_kernel's structure: persistent grid, GROUP lanes per row, non-temporal loads, ROWS::UNROLL row groups in flight, the f32 query
// slices in VGPRs, four f32x2 chains per query, DPP group sums, one WaveTopK list per wave and query, the workgroup rank merge,
// MIRROR_KP approximate keys per workgroup and query. A kernel declares its LDS, says where its queries are and calls mirror_pass; all
// of them run this one function, so a row's key for a query is the same whatever the query rode with and whether or not a bitmap was
// there. The certificates of the finish (mirror_finish.h) rest on that.
//
// ROWS, the row format (Bf16Rows, mirror_scan.hip), holds what a mirror's rows are (static members only):
//   Vec, UNROLL        the load vector (a lane owns 24 elements of a row: three Vec per row) and the row groups in flight
//   Side, side(p, r)   what a row carries beside its elements, loaded with them (nothing for bf16)
//   part(v, c)         the f32x2 that chain c multiplies, from one loaded Vec
//   start(q)           where the first chain starts
//   key<METRIC>(...)   the key distance from the group's sum
#pragma once
#include <cstddef>
#include <type_traits>

#include "kernels.h"
#include "row_math.h"
#include "topk.h"

namespace wax {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// The dimensions with a mirror pass: the BASELINE pair (three load vectors per lane and row divide them; kernel arguments hold the
// query). The exact re-score takes its lanes per row from ScanShape<DIMS> (row_math.h), like every exact path.
using MirrorDims = DimList<384, 768>;

constexpr int MIRROR_CAP = 128;                                                    // WaveTopK capacity
constexpr int MIRROR_PASS_LDS = SCAN_WAVES * MIRROR_CAP + SCAN_WAVES + MIRROR_KP;   // int64 words per query: lists, counts, merged

template <class ROWS, int DIMS>
struct MirrorShape {
    static constexpr int D8 = DIMS / 8;                // load vectors (8 elements) per row
    static constexpr int GROUP = D8 / 3, LOADS = 3;    // lanes per row; vectors per lane and row
    static constexpr int RPW = WAVE / GROUP, RPC = RPW * ROWS::UNROLL;   // rows per wave and load group; per wave iteration (a chunk)
    static_assert(D8 % GROUP == 0 && D8 / GROUP == LOADS, "three load vectors per lane and row");
};

// ---- where a pass finds its queries ----
// the lone query: floats in the kernel arguments (ARGSQ is the kernel's first argument: its offsets are the segment's), the rest in `a`
template <class ARGSQ>
struct LoneQuery {
    const MirrorScanArgs& a;
    static __device__ __forceinline__ const f32x4* kernarg_floats() {
        return reinterpret_cast<const f32x4*>((const char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(ARGSQ, q));
    }
    __device__ __forceinline__ const f32x4* floats(int) const { return kernarg_floats(); }
    __device__ __forceinline__ float norm(int) const { return a.q_norm; }
    __device__ __forceinline__ int64_t* partials(int) const { return a.partials; }
};
// the members of a shared pass: floats in device memory
struct MemberQueries {
    const MirrorMember* m;
    __device__ __forceinline__ const f32x4* floats(int i) const { return reinterpret_cast<const f32x4*>(m[i].query); }
    __device__ __forceinline__ float norm(int i) const { return m[i].q_norm; }
    __device__ __forceinline__ int64_t* partials(int i) const { return m[i].partials; }
    __device__ __forceinline__ const uint32_t* bitmap(int i) const { return m[i].bitmap; }   // (the masked 8-bit pass only)
};
// what the finish of member `m` gets: the shared arguments with the member's own lists, hits, certificate word, norm and k
__device__ __forceinline__ MirrorScanArgs member_args(MirrorScanArgs a, const MirrorMember& m) {
    a.partials = m.partials;
    a.hits = m.hits;
    a.certified = m.certified;
    a.q_norm = m.q_norm;
    a.k = m.k;
    a.kpad = m.kpad;
    return a;
}

// ---- the selection frame of a pass: the lists of one wave for the NQ queries, and their way into partials[blockIdx.x] ----
// What a pass does with its keys, spelled once: init, then per wave iteration room(rows) and one offer per query, then finish.
// Whatever FRAME says, the workgroup's partials are the MIRROR_KP smallest keys offered in the workgroup, ascending, KEY_PAD behind
// them: FRAME only chooses how the wave lists get there ("The selection frame").
//   SORTED  a list that a prune has left full keeps its first MIRROR_KP slots sorted from then on, so every later prune of it is
//           wave_prune_sorted (topk.h): the keys pushed since, ranked against a sorted prefix — less than half the broadcast reads
//           and compares of the general prune — and the final prune of a list that nothing was pushed to since is no prune at all.
//   Clock   hooks around the frame's phases; empty in every kernel of the library (tools/code8_shape_probe.hip times with them).
// No bound crosses a wave, let alone a workgroup: what a workgroup keeps depends on its own rows alone.
struct NoClock {
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void loop_begin() {}
    __device__ __forceinline__ void prune_in() {}
    __device__ __forceinline__ void prune_out() {}
    __device__ __forceinline__ void loop_end() {}
    __device__ __forceinline__ void done() {}
};
template <bool SORTED_, class CLOCK_ = NoClock>
struct PassFrame {
    static constexpr bool SORTED = SORTED_;
    using Clock = CLOCK_;
};
using FramePlain = PassFrame<false>;      // the frame as it was before PassLists: the general prune every time
using FrameShipped = PassFrame<true>;     // (profiles/r29: 0.604 against 0.620 ms for four queries over 10M x 384, 0.571 against 0.574 for one)

template <int NQ, class FRAME = FrameShipped>
struct PassLists {
    static_assert(NQ >= 1 && NQ <= MIRROR_MAX_NQ, "queries per pass");
    WaveTopK<MIRROR_CAP> tk[NQ];
    unsigned full;      // SORTED, bit i: a prune has left MIRROR_KP keys in list i
    int64_t* lds;
    int wave;
    typename FRAME::Clock clk;

    // `lds_`: NQ * MIRROR_PASS_LDS words of the kernel's
    __device__ __forceinline__ void init(int64_t* lds_, int wave_) {
        lds = lds_;
        wave = wave_;
#pragma unroll
        for (int i = 0; i < NQ; ++i) tk[i].init(lds + i * MIRROR_PASS_LDS + wave * MIRROR_CAP, MIRROR_KP);
        full = 0u;
    }

    // what a prune left, back in scalar registers (a noinline call returns in vector registers)
    __device__ __forceinline__ void pruned(int i, int cnt, int64_t tau) {
        tk[i].cnt = __builtin_amdgcn_readfirstlane(cnt);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)tau);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tau >> 32));
        tk[i].tau = (int64_t)(((uint64_t)hi << 32) | lo);
    }
    __device__ __forceinline__ void prune(int i) {
        if constexpr (FRAME::SORTED) {
            if ((full >> i) & 1u) {
                if (tk[i].cnt == MIRROR_KP) return;       // nothing pushed since the last prune: sorted as it stands
                const PruneOut r = wave_prune_sorted<MIRROR_CAP>((lds_i64*)tk[i].buf, tk[i].cnt);
                pruned(i, r.cnt, r.tau);
                return;
            }
        }
        const PruneOut r = wave_prune<MIRROR_CAP, true>((lds_i64*)tk[i].buf, tk[i].cnt, tk[i].k);
        pruned(i, r.cnt, r.tau);
        if constexpr (FRAME::SORTED) full |= (tk[i].cnt == MIRROR_KP ? 1u : 0u) << i;
    }

    // room for `rows` (<= MIRROR_CAP - MIRROR_KP) more keys in every list of the wave
    __device__ __forceinline__ void room(int rows) {
        bool shortof = false;
#pragma unroll
        for (int i = 0; i < NQ; ++i) shortof = shortof || tk[i].cnt > MIRROR_CAP - rows;
        if (shortof) {
            clk.prune_in();
#pragma unroll
            for (int i = 0; i < NQ; ++i)
                if (tk[i].cnt > MIRROR_CAP - rows) prune(i);
            clk.prune_out();
        }
    }

    // every lane of the wave, together: `key` to query i's list where `valid` (room() has made the room)
    __device__ __forceinline__ void offer(int i, int64_t key, bool valid) { tk[i].push(key, valid); }

    // per query: the waves' lists -> the workgroup's MIRROR_KP best -> partials(i)[blockIdx.x]; every thread of the workgroup
    template <class QUERIES>
    __device__ __forceinline__ void finish(const QUERIES& qs) {
        clk.loop_end();
        const int lane = lane_id();
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            prune(i);
            int* counts = reinterpret_cast<int*>(lds + i * MIRROR_PASS_LDS + SCAN_WAVES * MIRROR_CAP);
            if (lane == 0) counts[wave] = tk[i].cnt;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            int64_t* base = lds + i * MIRROR_PASS_LDS;
            block_rank_merge<SCAN_WAVES>(base, MIRROR_CAP, reinterpret_cast<int*>(base + SCAN_WAVES * MIRROR_CAP), MIRROR_KP,
                                         base + SCAN_WAVES * MIRROR_CAP + SCAN_WAVES);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int64_t* fin = lds + i * MIRROR_PASS_LDS + SCAN_WAVES * MIRROR_CAP + SCAN_WAVES;
            int64_t* mine = qs.partials(i) + (size_t)blockIdx.x * MIRROR_KP;
            for (int t = (int)threadIdx.x; t < MIRROR_KP; t += SCAN_THREADS) mine[t] = fin[t];
        }
        clk.done();
    }
};

// `lds`: NQ * MIRROR_PASS_LDS words of the kernel's. `bitmap` (MASKED; predicate.hip's: every word written, bits of rows >= n clear):
// the wave's chunk of RPC rows is the unit of the skip test, in scan_masked_kernel's form.
template <class ROWS, int DIMS, int METRIC, int NQ, bool MASKED, class QUERIES>
__device__ __forceinline__ void mirror_pass(const typename ROWS::Vec* __restrict__ rows, const typename ROWS::Side* __restrict__ sides,
                                            const MirrorScanArgs& a, const QUERIES& qs, const uint32_t* __restrict__ bitmap, int64_t* lds) {
    using S = MirrorShape<ROWS, DIMS>;
    constexpr int D8 = S::D8, GROUP = S::GROUP, LOADS = S::LOADS, RPW = S::RPW, RPC = S::RPC, UNROLL = ROWS::UNROLL;
    static_assert(NQ >= 1 && NQ <= MIRROR_MAX_NQ, "queries per pass");
    static_assert(!MASKED || ((RPC & (RPC - 1)) == 0 && RPC <= 32), "a chunk's bits must sit inside one bitmap word");

    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const int sub = lane / GROUP;
    const int gl = lane % GROUP;
    const bool owner = (gl == GROUP - 1);
    const uint32_t n = a.n_rows;

    // the query slices of this lane: elements [8c, 8c + 8) of vector c = gl + j * GROUP
    f32x2 q[NQ][LOADS][4];
    float start[NQ], qn[NQ], inv_qn[NQ];
    PassLists<NQ> lists;
    lists.init(lds, wave);
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const f32x4* q4 = qs.floats(i);
#pragma unroll
        for (int j = 0; j < LOADS; ++j) {
            const f32x4 lo = q4[2 * (gl + j * GROUP)], hi = q4[2 * (gl + j * GROUP) + 1];
            q[i][j][0] = lo.xy; q[i][j][1] = lo.zw; q[i][j][2] = hi.xy; q[i][j][3] = hi.zw;
        }
        start[i] = ROWS::start(q[i]);
        qn[i] = qs.norm(i);
        // cosine: mirror rows are unit vectors (or zero), so sim = acc / ||q||; the rule for a null query is the f32 scan's
        inv_qn[i] = qn[i] > COS_NORM_FLOOR ? 1.0f / qn[i] : 0.0f;
    }

    const uint32_t nchunks = (n + RPC - 1) / RPC;
    const uint32_t gwave = blockIdx.x * SCAN_WAVES + wave;
    const uint32_t nwaves = gridDim.x * SCAN_WAVES;

    uint32_t word = 0u, bits = 0u;
    if constexpr (MASKED) word = gwave < nchunks ? bitmap[(gwave * RPC) >> 5] : 0u;   // one iteration ahead
    for (uint32_t chunk = gwave; chunk < nchunks; chunk += nwaves) {
        if constexpr (MASKED) {
            const uint32_t r0 = chunk * RPC;                     // < n: word r0 >> 5 exists
            bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)((word >> (r0 & 31u)) & (uint32_t)((1ull << RPC) - 1ull)));
            const uint32_t next = chunk + nwaves;
            if (next < nchunks) word = bitmap[(next * RPC) >> 5];
            if (bits == 0u) continue;                            // wave-uniform: no row of the chunk may be offered, so none is loaded
        }
        const uint32_t rbase = chunk * RPC + sub;
        lists.room(RPC);
        typename ROWS::Vec v[UNROLL][LOADS];
        typename ROWS::Side side[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {                       // every load of the iteration is issued before the first product
            const uint32_t r = rbase + u * RPW;
            const uint32_t rc = r < n ? r : n - 1;               // clamp: tail lanes re-read the last row, result discarded
            const typename ROWS::Vec* p = rows + (size_t)rc * D8 + gl;
#pragma unroll
            for (int j = 0; j < LOADS; ++j) v[u][j] = __builtin_nontemporal_load(p + j * GROUP);
            side[u] = ROWS::side(sides, rc);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const uint32_t r = rbase + u * RPW;
            bool offer = owner && (r < n);
            if constexpr (MASKED) offer = offer && ((bits >> (uint32_t)(sub + u * RPW)) & 1u) != 0u;
#pragma unroll
            for (int i = 0; i < NQ; ++i) {                       // (the conversions are written per query; the compiler shares them)
                f32x2 acc[4] = {{start[i], 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
                for (int j = 0; j < LOADS; ++j) {
                    acc[0] = __builtin_elementwise_fma(q[i][j][0], ROWS::part(v[u][j], 0), acc[0]);
                    acc[1] = __builtin_elementwise_fma(q[i][j][1], ROWS::part(v[u][j], 1), acc[1]);
                    acc[2] = __builtin_elementwise_fma(q[i][j][2], ROWS::part(v[u][j], 2), acc[2]);
                    acc[3] = __builtin_elementwise_fma(q[i][j][3], ROWS::part(v[u][j], 3), acc[3]);
                }
                const f32x2 s2 = (acc[0] + acc[1]) + (acc[2] + acc[3]);
                const float s = group_sum<GROUP>(s2.x + s2.y);
                const float d = ROWS::template key<METRIC>(s, side[u], inv_qn[i], qn[i]);
                lists.offer(i, make_key(d + 0.0f, a.row_base + r), offer);
            }
        }
    }

    lists.finish(qs);
}

// ---- the host side of a pass ----
// scan_grid_for's large-store rule with the pass's rows per wave iteration: at most grid_cap (default 512 = 2 per CU) workgroups,
// every wave the same number of iterations (+-1 chunk in total)
inline int mirror_pass_grid(uint32_t n_rows, int rows_per_chunk, int grid_cap) {
    if (grid_cap <= 0) grid_cap = 512;
    if (grid_cap > SCAN_KWAY_MERGE_GRID) grid_cap = SCAN_KWAY_MERGE_GRID;
    const uint64_t rpc = (uint64_t)rows_per_chunk;
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

// What every launcher checks: the store's shape, and k and kpad of the lone query (m == nullptr: they are a's) or of each of nq members.
inline bool mirror_launch_ok(const MirrorScanArgs& a, int metric, int max_k, const MirrorMember* m = nullptr, int nq = 1) {
    if (!mirror_scan_supported(a.dims, metric) || a.n_rows == 0) return false;
    if (m == nullptr) return a.k >= 1 && a.k <= max_k && a.kpad >= a.k;
    if (nq < 2 || nq > MIRROR_MAX_NQ) return false;
    for (int i = 0; i < nq; ++i)
        if (m[i].k < 1 || m[i].k > max_k || m[i].kpad < m[i].k || m[i].query == nullptr) return false;
    return true;
}

// launch(ScanShape<dims>, metric constant, grid) at the instantiation of (dims, metric), with the grid of ROWS' pass at that dimension
template <class ROWS, typename F>
inline hipError_t with_mirror_pass(uint32_t n_rows, uint32_t dims, int metric, int grid_cap, F&& launch) {
    return with_scan_shape(MirrorDims{}, dims, [&](auto s) {
        return with_metric_in<M_COS, M_DOT>(metric, [&](auto m) {
            return launch(s, m, mirror_pass_grid(n_rows, MirrorShape<ROWS, decltype(s)::DIMS>::RPC, grid_cap));
        }, hipErrorInvalidValue);
    }, hipErrorInvalidValue);
}

// f(std::integral_constant<int, nq>{}) at the sizes of a shared pass (each has its own instantiation)
template <typename F>
inline hipError_t with_group_size(int nq, F&& f) {
    switch (nq) {
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        default: return hipErrorInvalidValue;
    }
}

// the second launch of every pass, behind the scan's (whose error, if any, is returned): `finish` with one workgroup per query
template <typename K, typename ARGS>
inline hipError_t launch_finish(K finish, int nq, hipStream_t st, const ARGS& args) {
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(finish, dim3(nq), dim3(SCAN_THREADS), 0, st, args);
    return hipGetLastError();
}

}  // namespace wax
