// batch_resident.hip — the exact batched search of a store that sits in L2 / MALL, in ONE launch per block of up to 1 024 queries.
//
// Who needs it: a store of thousands to tens of thousands of rows. The MFMA pipelines answer such a batch with a chain of launches
// (filter, survivors, re-score, select, finish) whose arithmetic is a few microseconds; the shared exact passes (multiscan.hip) keep
// per-wave threshold lists that never warm up on a share of a few hundred rows and put 16 queries on the machine per pass. Scoring
// EVERY (row, query) pair exactly in f32 costs less than either: no filter, no mirror, no certificate, no threshold.
//
// Split. Grid = row shares (x) x query blocks (y). A query block is up to 16 queries, staged once in LDS as float4 [16][D4]; a row
// share is a contiguous slice [share * n / shares, (share + 1) * n / shares) of the store, so no share is empty unless n < shares
// (such a workgroup writes empty lists). The host sizes the shares so that blocks x shares covers the CUs, up to the number of lists
// the finish merges in a round or two (batch_resident_shares).
//
// Distances are row_math.h's: lane g of a GROUP-lane group holds float4s g, g + GROUP, ... of a row, one fma chain per component
// (accumulate_dot / accumulate_norm), hsum, the summation tree of group_sum<GROUP> as a reduce-scatter (reduce_scatter.h: the same
// pairs are added, every lane ends with complete sums of different (query, row) pairs), finish_distance, make_key(d, row_base + row).
// Under cosine a row's norm is formed once per row-group and shared by its 16 queries. Rows come from the f32 store through the
// caches (plain loads: the query blocks re-read each other's rows from L2).
//
// Dense tile selection. A workgroup scores a tile of T rows (four waves, chunks of MS_U row-groups interleaved among them, the next
// chunk's rows requested before the current one is scored) against its 16 queries and writes all 16 x T keys to LDS. Then wave w
// takes queries w, w + 4, ...: the min(k, T) smallest keys of the query's tile by rank (wave_prune: every key counts the keys below
// it — no threshold, no per-wave list, nothing to warm up), rank-merged (two sorted lists, a binary search per key) into the ONE
// running best-k list the workgroup keeps per query. T balances the two costs per (row, query) pair — D / 4 float4 fmas against T
// compares — inside the LDS budget:
//
//   dims      T    queries [16][D4]   tile keys [16][256]   best-k [16][192]   total (+ 144 B of norms, ticket)
//   64      128          4 KB              32 KB                24 KB             60 KB
//   128     128          8 KB              32 KB                24 KB             64 KB
//   256     128         16 KB              32 KB                24 KB             72 KB
//   384     128         24 KB              32 KB                24 KB             80 KB
//   512     128         32 KB              32 KB                24 KB             88 KB
//   768     256         48 KB              32 KB                24 KB            104 KB
//   1024    256         64 KB              32 KB                24 KB            120 KB
//   1536    128         96 KB              32 KB                24 KB            152 KB   (of 160 KB: 16 queries fit at every dimension)
//
// The key area is 256 slots per query whatever T is: the finish reads whole partial lists (k <= 192) into it.
//
// Fused finish, no waiting. A workgroup publishes its 16 sorted lists to the workspace ([block][query][share][k], agent-scope
// write-through stores, drained before the workgroup barrier) and takes a ticket on its block's arrival counter (agent-scope RMW).
// The workgroup that completes the count re-reads the block's lists with agent-scope loads — scan_epilogue's hand-over (kernels.hip)
// — and, a wave per query, merges them: as many whole lists as fit the 256 key slots per round, rank-selected when a round holds
// several lists, rank-merged into the best-k list; then frame ids from the id table and out_stride hits per query, ascending,
// KEY_PAD / ID_PAD padded. It leaves the counter at zero for the next launch. No workgroup ever waits for another.
#include "kernels.h"
#include "reduce_scatter.h"
#include "row_math.h"
#include "topk.h"

namespace wax {

typedef __attribute__((address_space(3))) f32x4 lds_f32x4r;

constexpr int BR_KEYS = 256;            // key slots per query: a tile's keys (T <= 256) or whole partial lists (the finish)
constexpr int BR_BEST = FUSED_MAX_K;    // slots of a query's running best-k list

static constexpr int br_tile_rows(int d4) { return (d4 == 192 || d4 == 256) ? 256 : 128; }

// keys of lst[0 .. cnt) (ascending, cnt <= 192) below `key`: eight halvings end any search over fewer than 256 entries
__device__ inline int br_lower_bound(const lds_i64* lst, int cnt, int64_t key) {
    int lo = 0, hi = cnt;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const bool open = lo < hi;
        const int mid = open ? (lo + hi) >> 1 : 0;
        const bool before = lst[mid] < key;
        lo = (open && before) ? mid + 1 : lo;
        hi = (open && !before) ? mid : hi;
    }
    return lo;
}

// best[0 .. cb) and sel[0 .. cs): ascending, cb, cs <= k <= 192, no key in both. The k smallest of the two into best, ascending;
// returns their number. One wave, in place: every lane reads its keys and finds their ranks — own index plus the keys of the OTHER
// list below it — before any lane writes (a wave's DS instructions execute in order). Not inlined: cold code, as wave_prune.
__device__ __attribute__((noinline)) int br_wave_merge(lds_i64* best, int cb, const lds_i64* sel, int cs, int k) {
    constexpr int E = BR_BEST / 64;
    wave_lds_fence();
    if (cs == 0) return cb;
    if (cb == k && sel[0] > best[k - 1]) return cb;          // (wave-uniform) nothing of sel enters a full list
    const int lane = lane_id();
    int64_t b[E], s[E];
    int rb[E], rs[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int idx = lane + 64 * e;
        b[e] = idx < cb ? best[idx] : KEY_PAD;
        s[e] = idx < cs ? sel[idx] : KEY_PAD;
        rb[e] = rs[e] = k;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int idx = lane + 64 * e;
        if (64 * e < cb) rb[e] = idx + br_lower_bound(sel, cs, b[e]);
        if (64 * e < cs) rs[e] = idx + br_lower_bound(best, cb, s[e]);
    }
    wave_lds_fence();
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int idx = lane + 64 * e;
        if (idx < cb && rb[e] < k) best[rb[e]] = b[e];
        if (idx < cs && rs[e] < k) best[rs[e]] = s[e];
    }
    wave_lds_fence();
    return cb + cs < k ? cb + cs : k;
}

template <int D4, int GROUP, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS) void batch_resident_kernel(ResidentArgs a) {
    constexpr int LOADS = D4 / GROUP;
    constexpr int RPW = WAVE / GROUP;
    constexpr int RPC = RPW * MS_U;
    constexpr int T = br_tile_rows(D4);
    constexpr int LEVELS = GROUP == 64 ? 6 : (GROUP == 32 ? 5 : 4);
    constexpr int OUT = MS_M >> LEVELS;          // complete sums per lane per chunk: 4 / 2 / 1
    static_assert(D4 % GROUP == 0 && (GROUP == 16 || GROUP == 32 || GROUP == 64), "GROUP");
    static_assert(T % (RPC * SCAN_WAVES) == 0 && T <= BR_KEYS && MS_U == 4, "a tile is whole chunks of four row-groups");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    f32x4* qs = reinterpret_cast<f32x4*>(smem);                                        // [16][D4] (slots past the block's queries: zeros)
    int64_t* keys = reinterpret_cast<int64_t*>(smem + (size_t)MS_NQ * D4 * 16);        // [16][BR_KEYS]
    int64_t* best = keys + MS_NQ * BR_KEYS;                                            // [16][BR_BEST]
    float* qn_s = reinterpret_cast<float*>(best + MS_NQ * BR_BEST);                    // [16]
    int* ticket = reinterpret_cast<int*>(qn_s + MS_NQ);                                // [1]

    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const int sub = lane / GROUP;
    const int gl = lane % GROUP;
    const int k = (int)a.k;
    const uint32_t share = blockIdx.x, shares = gridDim.x, block = blockIdx.y;
    const uint32_t q0 = block * MS_NQ;
    const uint32_t nqb = a.nq - q0 < (uint32_t)MS_NQ ? a.nq - q0 : (uint32_t)MS_NQ;     // queries of this block (the grid has no empty block)
    const uint32_t begin = (uint32_t)((uint64_t)share * a.n_rows / shares);
    const uint32_t end = (uint32_t)((uint64_t)(share + 1) * a.n_rows / shares);

    if (begin < end) {
        for (uint32_t i = threadIdx.x; i < (uint32_t)MS_NQ * (uint32_t)D4; i += SCAN_THREADS) {
            const uint32_t qi = i / (uint32_t)D4, c = i - qi * (uint32_t)D4;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            qs[i] = qi < nqb ? reinterpret_cast<const f32x4*>(a.queries)[(size_t)(q0 + qi) * D4 + c] : zero;
        }
    }
    if (threadIdx.x < MS_NQ) qn_s[threadIdx.x] = threadIdx.x < nqb ? a.q_norm[q0 + threadIdx.x] : 0.f;
    __syncthreads();

    // the lane's selection bits and its query (reduce_scatter.h: value m = u * 16 + q, level L keeps bit L - 1 of m)
    const int b0 = lane & 1, b1 = (lane >> 1) & 1, b2 = (lane >> 2) & 1, b3 = (lane >> 3) & 1, b4 = (lane >> 4) & 1, b5 = (lane >> 5) & 1;
    const bool s1 = (b0 ^ b2) != 0, s2 = (b1 ^ b2) != 0, s3 = (b2 ^ b3) != 0, s4 = b3 != 0;
    const int q_lane = (s1 ? 1 : 0) | (s2 ? 2 : 0) | (s3 ? 4 : 0) | (s4 ? 8 : 0);
    const bool q_live = (uint32_t)q_lane < nqb;
    const float qn_lane = qn_s[q_lane];
    const int last_of_group = (lane & ~(GROUP - 1)) | (GROUP - 1);
    const f32x4* __restrict__ store4 = reinterpret_cast<const f32x4*>(a.store);
    const lds_f32x4r* qs_l = (const lds_f32x4r*)qs + gl;
    lds_i64* keys_lane = (lds_i64*)keys + (size_t)q_lane * BR_KEYS;

    int cb[MS_NQ / SCAN_WAVES];                  // live keys of the best-k lists of this wave's queries (wave-uniform)
#pragma unroll
    for (int i = 0; i < MS_NQ / SCAN_WAVES; ++i) cb[i] = 0;

    for (uint32_t tile0 = begin; tile0 < end; tile0 += (uint32_t)T) {
        const uint32_t live = end - tile0 < (uint32_t)T ? end - tile0 : (uint32_t)T;
        const uint32_t nch = (live + RPC - 1) / RPC;
        // chunk ci: row-groups u = 0 .. 3 of rows tile0 + ci * RPC + sub + u * RPW; rows past the share re-read its last row, unused
        auto load_chunk = [&](f32x4 (&v)[MS_U][LOADS], uint32_t ci) {
            const uint32_t rbase = tile0 + ci * RPC + sub;
#pragma unroll
            for (int u = 0; u < MS_U; ++u) {
                const uint32_t r = rbase + u * RPW;
                const uint32_t rc = r < end ? r : end - 1;
                const f32x4* p = store4 + (size_t)rc * D4 + gl;
#pragma unroll
                for (int j = 0; j < LOADS; ++j) v[u][j] = p[j * GROUP];
            }
        };
        auto score_chunk = [&](const f32x4 (&v)[MS_U][LOADS], uint32_t ci) {
            const uint32_t rbase = tile0 + ci * RPC + sub;
            // ||v||^2 once per row-group (the norm half of finish_row), handed to every lane of the group
            auto row_norm = [&](const f32x4 (&vu)[LOADS]) -> float {
                if (METRIC != M_COS) return 0.f;
                f32x4 nrm = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < LOADS; ++j) accumulate_norm(vu[j], nrm);
                const float tot = group_sum<GROUP>(hsum(nrm));                   // valid in the group's last lane
                return __shfl(tot, last_of_group, 64);
            };
            const float nb0 = row_norm(v[0]), nb1 = row_norm(v[1]), nb2 = row_norm(v[2]), nb3 = row_norm(v[3]);
            // lane-private partial sums of all 64 (row-group, query) pairs; a query's slice comes from LDS one query ahead
            float part[MS_M];
            f32x4 qa[LOADS], qb[LOADS];
#pragma unroll
            for (int j = 0; j < LOADS; ++j) qa[j] = qs_l[j * GROUP];
#pragma unroll
            for (int qi = 0; qi < MS_NQ; ++qi) {
                const int qnext = qi + 1 < MS_NQ ? qi + 1 : qi;
#pragma unroll
                for (int j = 0; j < LOADS; ++j) qb[j] = qs_l[(size_t)qnext * D4 + j * GROUP];
#pragma unroll
                for (int u = 0; u < MS_U; ++u) {
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int j = 0; j < LOADS; ++j) accumulate_dot<METRIC>(qa[j], v[u][j], acc);
                    part[u * MS_NQ + qi] = hsum(acc);
                }
#pragma unroll
                for (int j = 0; j < LOADS; ++j) qa[j] = qb[j];
            }
            ms_halve<0xB1, MS_M>(part, s1);           // quad_perm [1,0,3,2]
            ms_halve<0x4E, MS_M / 2>(part, s2);       // quad_perm [2,3,0,1]
            ms_halve<0x141, MS_M / 4>(part, s3);      // row_half_mirror
            ms_halve<0x140, MS_M / 8>(part, s4);      // row_mirror
            if (GROUP >= 32) ms_halve_rows16<MS_M / 16>(part);
            if (GROUP >= 64) ms_halve_rows32<MS_M / 32>(part);
            // the lane owns OUT complete sums, all of query q_lane: row-group u of value index j << LEVELS | (selection bits)
#pragma unroll
            for (int j = 0; j < OUT; ++j) {
                int u;
                float nrm;
                if (GROUP == 16) { u = j; nrm = j == 0 ? nb0 : (j == 1 ? nb1 : (j == 2 ? nb2 : nb3)); }
                else if (GROUP == 32) { u = b4 + 2 * j; nrm = j == 0 ? (b4 ? nb1 : nb0) : (b4 ? nb3 : nb2); }
                else { u = b4 + 2 * b5; nrm = b5 ? (b4 ? nb3 : nb2) : (b4 ? nb1 : nb0); }
                const float d = finish_distance<METRIC>(part[j], nrm, qn_lane);
                const uint32_t r = rbase + (uint32_t)u * RPW;
                if (q_live && r < end) keys_lane[r - tile0] = make_key(d, a.row_base + r);      // r - tile0 < live <= T
            }
        };
        uint32_t ci = (uint32_t)wave;
        if (ci < nch) {
            f32x4 va[MS_U][LOADS], vb[MS_U][LOADS];
            load_chunk(va, ci);
            for (;;) {
                const uint32_t nx = ci + SCAN_WAVES;
                load_chunk(vb, nx < nch ? nx : ci);       // unconditional: past the end it re-requests the current chunk
                __builtin_amdgcn_sched_barrier(0);        // the requests go out before the first use of the current set
                score_chunk(va, ci);
                if (nx >= nch) break;
                ci = nx;
#pragma unroll
                for (int u = 0; u < MS_U; ++u) {
#pragma unroll
                    for (int j = 0; j < LOADS; ++j) va[u][j] = vb[u][j];
                }
            }
        }
        __syncthreads();
        // dense selection: the tile's min(k, live) smallest keys of a query by rank, merged into its running list
#pragma unroll
        for (int i = 0; i < MS_NQ / SCAN_WAVES; ++i) {
            const int q = wave + SCAN_WAVES * i;
            if ((uint32_t)q >= nqb) continue;
            lds_i64* kq = (lds_i64*)keys + (size_t)q * BR_KEYS;
            const PruneOut pr = wave_prune<T, true>(kq, (int)live, k);
            cb[i] = br_wave_merge((lds_i64*)best + (size_t)q * BR_BEST, cb[i], kq, pr.cnt, k);
        }
        __syncthreads();                                  // the next tile rewrites the key area
    }

    // publish: this workgroup's list of query q at partials[((q0 + q) * shares + share) * k], KEY_PAD behind its keys
#pragma unroll
    for (int i = 0; i < MS_NQ / SCAN_WAVES; ++i) {
        const int q = wave + SCAN_WAVES * i;
        if ((uint32_t)q >= nqb) continue;
        for (int t = cb[i] + lane; t < k; t += WAVE) best[(size_t)q * BR_BEST + t] = KEY_PAD;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nqb * (uint32_t)k; i += SCAN_THREADS) {
        const uint32_t q = i / (uint32_t)k, t = i - q * (uint32_t)k;
        __hip_atomic_store(a.partials + ((size_t)(q0 + q) * shares + share) * (size_t)k + t, best[(size_t)q * BR_BEST + t], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing wave drains before the ticket
    __syncthreads();
    if (threadIdx.x == 0) *ticket = (int)__hip_atomic_fetch_add(a.arrive + block, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if ((uint32_t)*ticket != shares - 1u) return;

    // the last arriver of this query block: a wave per query, the block's lists in share order (whoever arrives last, the same steps)
    const int per = 2 * k <= BR_KEYS ? BR_KEYS / k : 1;   // whole lists per round of BR_KEYS slots
#pragma unroll 1
    for (int q = wave; (uint32_t)q < nqb; q += SCAN_WAVES) {
        lds_i64* kq = (lds_i64*)keys + (size_t)q * BR_KEYS;
        lds_i64* bq = (lds_i64*)best + (size_t)q * BR_BEST;
        const int64_t* lists = a.partials + (size_t)(q0 + q) * shares * (size_t)k;
        int have = 0;
        for (uint32_t sh0 = 0; sh0 < shares; sh0 += (uint32_t)per) {
            const int nl = shares - sh0 < (uint32_t)per ? (int)(shares - sh0) : per;
            const int total = nl * k;                     // <= BR_KEYS
            int fresh = 0;
            wave_lds_fence();
#pragma unroll
            for (int e = 0; e < BR_KEYS / 64; ++e) {
                const int idx = lane + 64 * e;
                const int64_t key = idx < total ? __hip_atomic_load(lists + (size_t)sh0 * k + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : KEY_PAD;
                if (idx < total) kq[idx] = key;
                fresh += __popcll(__ballot(key != KEY_PAD));
            }
            if (fresh == 0) continue;                     // (wave-uniform) empty shares
            // several lists: their k smallest by rank (the padding keys rank behind every live key); one list is sorted as it is
            if (nl > 1) (void)wave_prune<BR_KEYS, true>(kq, total, k);
            have = br_wave_merge(bq, have, kq, fresh < k ? fresh : k, k);
        }
        wave_lds_fence();
        wax_hip_hit* out = a.out + (size_t)(q0 + q) * a.out_stride;
        for (uint32_t t = (uint32_t)lane; t < a.out_stride; t += WAVE) {
            wax_hip_hit h;
            h.key = (int)t < have ? bq[t] : KEY_PAD;
            h.frame_id = ID_PAD;
            if (h.key != KEY_PAD) {
                const uint32_t local = key_row(h.key) - a.row_base;
                h.frame_id = (a.ids != nullptr && local < a.n_rows) ? a.ids[local] : (uint64_t)key_row(h.key);
            }
            out[t] = h;
        }
    }
    if (threadIdx.x == 0) __hip_atomic_store(a.arrive + block, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------
// launch side: every specialised dimension of row_math.h's table

bool batch_resident_dims(uint32_t dims) { return scan_group_lanes(dims) != 0; }

uint32_t batch_resident_tile_rows(uint32_t dims) { return batch_resident_dims(dims) ? (uint32_t)br_tile_rows((int)(dims / 4)) : 0u; }

size_t batch_resident_lds_bytes(uint32_t dims) {
    return (size_t)MS_NQ * dims * 4 + (size_t)MS_NQ * BR_KEYS * 8 + (size_t)MS_NQ * BR_BEST * 8 + (size_t)MS_NQ * 4 + 16;
}

// Row shares of a launch of `blocks` query blocks on `cus` compute units: enough workgroups to cover the CUs, but no more lists per
// query than the finish takes in two rounds of BR_KEYS keys (a round is a rank selection of 256 keys by one wave, ~2 us; the
// shares' own work shrinks with their number, the finish grows with it) — at least 8, at most 64.
uint32_t batch_resident_shares(uint32_t blocks, int k, uint32_t cus) {
    if (blocks < 1) blocks = 1;
    uint32_t cap = (uint32_t)(2 * BR_KEYS / (k < 1 ? 1 : k));
    cap = cap < 8 ? 8 : (cap > 64 ? 64 : cap);
    const uint32_t want = (cus + blocks - 1) / blocks;
    return want < 1 ? 1 : (want > cap ? cap : want);
}

template <int D4, int GROUP, int METRIC>
static hipError_t br_launch_one(const ResidentArgs& a, dim3 grid, size_t smem, hipStream_t st) {
    static std::atomic<uint64_t> configured{0};   // per device (ensure_dynamic_lds)
    if (smem > 64 * 1024) {
        hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&batch_resident_kernel<D4, GROUP, METRIC>), 160 * 1024, configured);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((batch_resident_kernel<D4, GROUP, METRIC>), grid, dim3(SCAN_THREADS), smem, st, a);
    return hipGetLastError();
}

hipError_t launch_batch_resident(const ResidentArgs& a, uint32_t dims, int metric, uint32_t shares, hipStream_t st) {
    if (!batch_resident_dims(dims) || a.k < 1 || a.k > (uint32_t)FUSED_MAX_K || a.nq < 1 || a.nq > RESIDENT_MAX_Q || shares < 1 || a.n_rows < 1 ||
        a.out_stride < 1 || !a.store || !a.queries || !a.q_norm || !a.partials || !a.arrive || !a.out)
        return hipErrorInvalidValue;
    const size_t smem = batch_resident_lds_bytes(dims);
    if (smem > 160 * 1024) return hipErrorInvalidValue;
    const dim3 grid(shares, (a.nq + MS_NQ - 1) / MS_NQ);
    return with_scan_shape(dims, [&](auto s) {
        using S = decltype(s);
        return with_metric(metric, [&](auto m) { return br_launch_one<S::D4, S::GROUP, decltype(m)::value>(a, grid, smem, st); }, hipErrorInvalidValue);
    }, hipErrorInvalidValue);
}

}  // namespace wax
