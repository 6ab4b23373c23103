// mirror8_dims.hip — up to four cosine or dot queries against the 8-bit code mirror of a 512-, 1 024- or 1 536-d store in one pass on
// v_mfma_i32_16x16x64_i8, optionally under a row bitmap, answered in f32 ("The code mirror at 512, 1 024 and 1 536
// dimensions"; wax_hip_search_mirror_codes, api_mirror8_dims.inc).
//
// What stays mirror8_scan.hip's, to the letter (mirror8_code.h, mirror8_layout.h, mirror_pass.h): the codes and their 16-row tiles in
// operand order, the +128 bias taken off by one v_xor per dword, the query as three balanced base-128 digits per element, operand B's
// 16 columns = (query, plane), exact integer plane sums, code8_sum and code8_key as the one float epilogue, Mirror8Slack, PassLists,
// the persistent grid, the clamp of tail rows, and the masked form's rule (a tile whose 16 bits are zero for every live member is
// skipped before its loads; a lane offers only where its own query's bit is set; the sums never see the bitmap). The integer sums
// are exact and the epilogue is one function of (S, delta, meta, norm), so a row's key for a query is the same alone and in a pass of
// 2, 3 or 4.
//
// What is new is the split. code8_pass keeps a tile's codes AND the query's digits in registers, KSTEPS x 4 VGPRs each (KSTEPS = D / 64):
// 96 + 96 at 1 536-d. Here
//   the digits  are prepared ONCE per workgroup — wave w quantises k-steps w, w + 4, ... for all four waves, a quarter of
//               code8_pass's prologue per wave — into LDS in operand-B order: dig[s][lane] is the 16 bytes lane `lane` multiplies
//               at k-step s, 1 KB per k-step (8 / 16 / 24 KB), read back with one conflict-free ds_read_b128 per MFMA;
//   the codes   stream through two register buffers of PIECE = 8 k-steps (32 VGPRs, 128 B per lane each): the next piece's
//               non-temporal global_load_dwordx4s are issued before the current piece's MFMAs, and the next tile's first piece
//               before the current tile's epilogue, so 128 B per lane are in flight under every MFMA run and under the selection
//               frame (code8_pass at 384-d: 96 B, and nothing under its epilogue). At 512-d a tile is one piece and at
//               1 536-d three: the piece prefetched behind an odd number of pieces is moved to the first buffer (32 v_mov).
// Rejected: digits in registers with K split across the waves of a pair (batch_ksplit.hip's hand-over) — each wave still holds D / 128
// k-steps of digits (48 VGPRs at 1 536-d) and every tile costs an LDS round trip and a barrier between waves that the persistent
// loop otherwise never needs; two accumulators over two tiles to hide the ds_read latency — the reads of a piece are independent of
// its loads and are issued ahead of the MFMAs by the scheduler, and a second tile in flight doubles the code buffers for nothing.
//
// Resources (the compiler's report at the build's flags, gfx950, -O3, no packed f32; lone .. four-query kernels, masked or not):
// 512-d 115 - 122 VGPRs, 67 - 100 SGPRs, 4 waves per SIMD; 1 024-d 104 - 112 VGPRs, 69 - 102 SGPRs, 4 waves; 1 536-d 116 - 128 VGPRs,
// 72 - 106 SGPRs, 4 waves (four queries: 3, by its 42 KB of LDS). ScratchSize 0, VGPRs Spill 0 and SGPRs Spill 0 in every kernel of
// the unit, the re-score (57 - 132 VGPRs) and the finish (13) included. LDS: 4 640 B of lists per query + 8 / 16 / 24 KB of digits.
//
// The finish. Lower bounds spread as 1 / sqrt(D) while a row's err stays near 0.008, so the 64 candidates of mirror_finish do not
// certify here (tests/test_mirror8_dims_gpu.py restates the model). The pass is followed by mirror_wide.hip's selection, one workgroup
// per member — B = min(T, K_C), C = MIRROR8_DIMS_C = 128, the smallest count the model clears ten slacks with — then
//   mirror8_dims_rescore_kernel  row_distance at ScanShape<DIMS> for every candidate of every member (the f32 scan's bits), the query
//                                read from device memory (1 536 floats do not fit the kernel arguments beside the members),
//   mirror8_dims_finish_kernel   one workgroup per member: the exact keys sorted in LDS, the hits, the certificate
//                                B == KEY_PAD (every row was re-scored) or dist(B) - Mirror8Slack > d_k, strict.
// Mirror8Slack's terms are written for any D (mirror_finish.h): (a) scales with sqrt(D) on both sides of its inequality, (b) is 3 D u
// by definition, (c) does not depend on D. The plane sums stay exact in f32: D * 64 * 127 < 2^24 up to 2 064-d (asserted below).
#include <cstring>

#include "mirror8_code.h"
#include "mirror8_layout.h"
#include "mirror_finish.h"
#include "mirror_pass.h"

namespace wax {

namespace {

template <int DIMS>
struct Code8Pieces {
    static constexpr int TILE = 16;                    // rows per MFMA and per wave iteration
    static constexpr int KSTEPS = DIMS / 64;           // MFMAs per tile
    static constexpr int PIECE = 8;                    // k-steps per register buffer: 128 B per lane in flight
    static constexpr int NPIECES = KSTEPS / PIECE;
    static_assert(DIMS % (64 * PIECE) == 0 && KSTEPS % SCAN_WAVES == 0, "whole pieces; every wave prepares the same number of k-steps");
    static_assert((long long)DIMS * 64 * 127 < (1ll << 24), "a plane sum must be an exact f32");
    static_assert(TILE == (int)MIRROR8_TILE_ROWS && TILE <= MIRROR_CAP - MIRROR_KP, "the layout's tile; a tile fits the room of a pruned list");
};

// `dig`: KSTEPS * 64 operand-B vectors of the workgroup's; `lds`: NQ * MIRROR_PASS_LDS words.
template <int DIMS, int METRIC, int NQ, bool MASKED>
__device__ __forceinline__ void code8_dims_pass(const unsigned char* __restrict__ codes, const f32x2* __restrict__ sides, const MirrorScanArgs& a,
                                                const MemberQueries& qs, i32x4* dig, int64_t* lds) {
    using T = Code8Pieces<DIMS>;
    constexpr int KSTEPS = T::KSTEPS, TILE = T::TILE, PIECE = T::PIECE, NPIECES = T::NPIECES;
    static_assert(NQ >= 1 && NQ <= MIRROR_MAX_NQ && MIRROR_MAX_NQ * 4 <= 16, "four columns per query");

    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const int col = lane & 15, kg = lane >> 4;        // operand A: row col of the tile, bytes 16 kg of every 64; operand B: column col
    const int myq = col >> 2, plane = col & 3;        // the query and plane of this lane's column; after the combine: row 4 kg + plane
    const bool live = myq < NQ;
    const uint32_t n = a.n_rows;
    const uint32_t nchunks = (n + TILE - 1) / TILE;
    const uint32_t gwave = blockIdx.x * SCAN_WAVES + wave;
    const uint32_t nwaves = gridDim.x * SCAN_WAVES;

    PassLists<NQ> lists;
    lists.init(lds, wave);

    // this lane's query: delta and the norm; the digits of its plane go to LDS, a quarter of the k-steps per wave
    float delta = 0.f, qn = 0.f;
    const float* mine = reinterpret_cast<const float*>(qs.floats(0));
    const uint32_t* my_bitmap = nullptr;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const float di = query_delta<DIMS>(qs.floats(i), lane);
        if (myq == i) { delta = di; qn = qs.norm(i); mine = reinterpret_cast<const float*>(qs.floats(i)); }
        if constexpr (MASKED) { if (myq == i) my_bitmap = qs.bitmap(i); }
    }
    // cosine: mirror rows are unit vectors (or zero), so sim = s / ||q||; the rule for a null query is the f32 scan's
    const float inv_qn = qn > COS_NORM_FLOOR ? 1.0f / qn : 0.0f;
    const float inv_delta = delta > 0.f ? __fdiv_rn(1.0f, delta) : 0.f;      // (delta = 0 or NaN: no digits)
    for (int j = 0; j < KSTEPS / SCAN_WAVES; ++j) {
        const int s = j * SCAN_WAVES + wave;
        dig[s * WAVE + lane] = query_digits(mine + s * 64 + kg * 16, inv_delta, live ? plane : 3);
    }
    __syncthreads();

    // the word of this lane's query that holds tile c's bits (c < nchunks: row 16 c < n, so word c >> 1 exists)
    auto tile_word = [&](uint32_t c) -> uint32_t { return !live ? 0u : my_bitmap == nullptr ? 0xffffffffu : my_bitmap[c >> 1]; };
    // the first tile at or behind c (in this wave's walk) of which some live member may be offered a row, and this lane's 16 bits
    // of it; nchunks or more: none. The ballot makes the test wave-uniform.
    auto advance = [&](uint32_t c, uint32_t& bits) -> uint32_t {
        if constexpr (MASKED) {
            while (c < nchunks) {
                bits = (tile_word(c) >> ((c & 1u) * 16u)) & 0xffffu;
                if (__ballot(bits != 0u) != 0ull) break;
                c += nwaves;
            }
        }
        return c;
    };
    // piece pc of a tile: k-steps [PIECE pc, PIECE pc + PIECE), 1 024 contiguous bytes per wave load. The clamp makes tail lanes
    // re-read the last row: no byte that the writer did not write reaches a key.
    auto load_piece = [&](u32x4 (&v)[PIECE], uint32_t chunk, int pc) {
        const uint32_t ra = chunk * TILE + col;
        const uint32_t rc = ra < n ? ra : n - 1;
        const unsigned char* p = codes + mirror8_offset(rc, 64 * PIECE * pc + 16 * kg, DIMS);
#pragma unroll
        for (int s = 0; s < PIECE; ++s) v[s] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + 1024 * s));
    };

    uint32_t bits = 0xffffu, next_bits = 0xffffu;
    uint32_t chunk = advance(gwave, bits);
    u32x4 v0[PIECE], v1[PIECE];
    if (chunk < nchunks) load_piece(v0, chunk, 0);

    // one tile whose first piece is in flight in v0; leaves the next tile's first piece in flight in v0 (even pieces sit in v0, odd
    // ones in v1: behind an odd number of pieces the prefetched buffer is moved over, 32 v_mov per tile — a second copy of the
    // body with the buffers swapped spares them and costs 30 VGPRs at 512-d and two spilled SGPRs at 1 536-d)
    auto tile = [&]() {
        const uint32_t next = advance(chunk + nwaves, next_bits);
        const uint32_t r = chunk * TILE + 4 * kg + plane;                        // the row this lane will hold the key of
        const f32x2 side = __builtin_nontemporal_load(sides + (r < n ? r : n - 1));
        lists.room(TILE);
        i32x4 acc = {0, 0, 0, 0};
#pragma unroll
        for (int pc = 0; pc < NPIECES; ++pc) {
            auto& cur = (pc & 1) ? v1 : v0;
            auto& nxt = (pc & 1) ? v0 : v1;
            if (pc + 1 < NPIECES) load_piece(nxt, chunk, pc + 1);
            else if (next < nchunks) load_piece(nxt, next, 0);
#pragma unroll
            for (int s = 0; s < PIECE; ++s) {
                const i32x4 b = dig[(pc * PIECE + s) * WAVE + lane];
                const u32x4 x = cur[s] ^ 0x80808080u;
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, x), b, acc, 0, 0, 0);
            }
        }
        float S = 0.f;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const float pl = (float)acc[reg];
            const float Sr = code8_sum(quad_bcast<0>(pl), quad_bcast<1>(pl), quad_bcast<2>(pl));
            S = plane == reg ? Sr : S;
        }
        const float d = code8_key<METRIC>(S, delta, side, inv_qn, qn);
        bool offer = live && r < n;
        if constexpr (MASKED) offer = offer && ((bits >> (uint32_t)(4 * kg + plane)) & 1u) != 0u;
        const int64_t key = make_key(d + 0.0f, a.row_base + r);
#pragma unroll
        for (int i = 0; i < NQ; ++i) lists.offer(i, key, offer && myq == i);
        if constexpr ((NPIECES & 1) != 0) {
#pragma unroll
            for (int s = 0; s < PIECE; ++s) v0[s] = v1[s];
        }
        chunk = next;
        bits = next_bits;
    };
    while (chunk < nchunks) tile();

    lists.finish(qs);
}

}  // namespace

template <int DIMS, int METRIC, int NQ, bool MASKED>
__global__ __launch_bounds__(SCAN_THREADS, 2) void mirror8_dims_pass_kernel(Mirror8GroupArgs ga) {
    __shared__ int64_t lds[NQ * MIRROR_PASS_LDS];
    __shared__ i32x4 dig[Code8Pieces<DIMS>::KSTEPS * WAVE];
    code8_dims_pass<DIMS, METRIC, NQ, MASKED>(ga.codes, reinterpret_cast<const f32x2*>(ga.meta), ga.g.a, MemberQueries{ga.g.m}, dig, lds);
}

// rows of one wave in flight in the re-score, and the candidates of a workgroup (GROUP is 64 at all three dimensions: a wave per row)
constexpr int DIMS_FLIGHT = 4;
template <int DIMS>
struct Rescore8Shape {
    static constexpr int GROUP = ScanShape<DIMS>::GROUP, RPW = WAVE / GROUP;
    static constexpr int ROWS_PER_STEP = RPW * SCAN_WAVES, ROWS_PER_BLOCK = ROWS_PER_STEP * DIMS_FLIGHT;
    static_assert(MIRROR8_DIMS_C % ROWS_PER_BLOCK == 0, "whole workgroups");
};

// grid (C / ROWS_PER_BLOCK, members): candidates [base, base + ROWS_PER_BLOCK) of member blockIdx.y
template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS) void mirror8_dims_rescore_kernel(Mirror8DimsArgs d) {
    constexpr int D4 = ScanShape<DIMS>::D4, GROUP = ScanShape<DIMS>::GROUP, LOADS = ScanShape<DIMS>::LOADS;
    constexpr int RPW = Rescore8Shape<DIMS>::RPW, STEP = Rescore8Shape<DIMS>::ROWS_PER_STEP, BLOCK = Rescore8Shape<DIMS>::ROWS_PER_BLOCK;
    const MirrorScanArgs& a = d.ga.g.a;
    const MirrorMember& mb = d.ga.g.m[blockIdx.y];
    const int64_t* cand = d.cand + (size_t)blockIdx.y * MIRROR8_DIMS_C;
    int64_t* exact = d.exact + (size_t)blockIdx.y * MIRROR8_DIMS_C;
    const int t = (int)threadIdx.x, lane = lane_id(), wave = t >> 6;
    const uint32_t m = (uint32_t)d.ctl[(size_t)blockIdx.y * MIRROR_WIDE_CTL];
    const uint32_t base = blockIdx.x * (uint32_t)BLOCK;              // (the grid is C / BLOCK: base + BLOCK <= C)
    if (base >= m) {                                                 // a workgroup without a candidate: dead slots
        if (t < BLOCK) exact[base + t] = KEY_PAD;
        return;
    }
    const f32x4* q4 = reinterpret_cast<const f32x4*>(mb.query);
    const int sub = lane / GROUP, gl = lane % GROUP;
    f32x4 q[LOADS];
#pragma unroll
    for (int j = 0; j < LOADS; ++j) q[j] = q4[gl + j * GROUP];
    const f32x4* __restrict__ store4 = reinterpret_cast<const f32x4*>(a.store);
    f32x4 v[DIMS_FLIGHT][LOADS];
    bool live[DIMS_FLIGHT];
    uint32_t grow[DIMS_FLIGHT];
#pragma unroll
    for (int p = 0; p < DIMS_FLIGHT; ++p) {      // every load of the wave in flight before the first product
        const uint32_t i = base + (uint32_t)(p * STEP + wave * RPW + sub);
        const int64_t key = cand[i];
        grow[p] = key_row(key);
        const uint32_t lrow = grow[p] - a.row_base;
        live[p] = i < m && key != KEY_PAD && lrow < a.n_rows;
        const f32x4* src = store4 + (size_t)(live[p] ? lrow : 0u) * D4 + gl;
#pragma unroll
        for (int j = 0; j < LOADS; ++j) v[p][j] = src[j * GROUP];
    }
#pragma unroll
    for (int p = 0; p < DIMS_FLIGHT; ++p) {
        const float dist = row_distance<GROUP, LOADS, METRIC>(q, v[p], mb.q_norm);
        if (gl == GROUP - 1) exact[base + (uint32_t)(p * STEP + wave * RPW + sub)] = live[p] ? make_key(dist, grow[p]) : KEY_PAD;
    }
}

// one workgroup per member: mirror_wide_finish_kernel's sort, hits and certificate at C = MIRROR8_DIMS_C under Mirror8Slack
template <int DIMS, int METRIC>
__global__ __launch_bounds__(MERGE_THREADS) void mirror8_dims_finish_kernel(Mirror8DimsArgs d) {
    __shared__ int64_t keys[MIRROR8_DIMS_C];
    const MirrorScanArgs a = member_args(d.ga.g.a, d.ga.g.m[blockIdx.x]);
    const int64_t* exact = d.exact + (size_t)blockIdx.x * MIRROR8_DIMS_C;
    const uint64_t* ctl = d.ctl + (size_t)blockIdx.x * MIRROR_WIDE_CTL;
    const int t = (int)threadIdx.x;
    const uint32_t m = (uint32_t)ctl[0];
    uint32_t n = WAVE;                                   // the sort's size: a power of two >= m, <= C (C is one)
    while (n < m) n <<= 1;
    if (n > (uint32_t)MIRROR8_DIMS_C) n = (uint32_t)MIRROR8_DIMS_C;
    for (uint32_t i = (uint32_t)t; i < n; i += MERGE_THREADS) keys[i] = exact[i];
    __syncthreads();
    // bitonic sort, ascending (live keys are unique; the pads end up behind them)
    for (uint32_t span = 2u; span <= n; span <<= 1) {
        for (uint32_t j = span >> 1; j > 0u; j >>= 1) {
            for (uint32_t i = (uint32_t)t; i < n; i += MERGE_THREADS) {
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
    for (int i = t; i < a.kpad; i += MERGE_THREADS) {
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
        const int64_t B = (int64_t)ctl[2];
        bool ok = B == KEY_PAD;                          // every listed row is every row that may be offered, and each was re-scored
        if (!ok && m >= (uint32_t)a.k) {
            const float eps = Mirror8Slack::template eps<DIMS, METRIC>(a);
            const int64_t kth = keys[a.k - 1];
            const float db = key_distance(B), dk = key_distance(kth);
            ok = kth != KEY_PAD && __builtin_isfinite(db) && __builtin_isfinite(dk) && __builtin_isfinite(eps) && a.q_norm == a.q_norm &&
                 (db - eps > dk);                        // strict: ties stay uncertified
        }
        *a.certified = ok ? 1u : 0u;
    }
}

bool mirror8_dims_supported(uint32_t dims, int metric) {
    return in_dim_list(Mirror8WideDims{}, dims) && (metric == M_COS || metric == M_DOT);
}

int mirror8_dims_grid(uint32_t n_rows, uint32_t dims, int grid_cap) {
    return mirror8_dims_supported(dims, M_COS) && n_rows != 0u ? mirror_pass_grid(n_rows, (int)MIRROR8_TILE_ROWS, grid_cap) : 0;
}

namespace {
template <int DIMS, int METRIC, bool MASKED>
void launch_pass8(const Mirror8GroupArgs& ga, int nq, int grid, hipStream_t st) {
    switch (nq) {
        case 1: launch_kernel((mirror8_dims_pass_kernel<DIMS, METRIC, 1, MASKED>), dim3(grid), dim3(SCAN_THREADS), 0, st, ga); break;
        case 2: launch_kernel((mirror8_dims_pass_kernel<DIMS, METRIC, 2, MASKED>), dim3(grid), dim3(SCAN_THREADS), 0, st, ga); break;
        case 3: launch_kernel((mirror8_dims_pass_kernel<DIMS, METRIC, 3, MASKED>), dim3(grid), dim3(SCAN_THREADS), 0, st, ga); break;
        default: launch_kernel((mirror8_dims_pass_kernel<DIMS, METRIC, 4, MASKED>), dim3(grid), dim3(SCAN_THREADS), 0, st, ga); break;
    }
}
}  // namespace

hipError_t launch_mirror8_dims(const Mirror8DimsArgs& args, int nq, int metric, int grid_cap, hipStream_t st) {
    const MirrorScanArgs& a = args.ga.g.a;
    if (nq < 1 || nq > MIRROR_MAX_NQ || !mirror8_dims_supported(a.dims, metric) || a.n_rows == 0u || args.ga.codes == nullptr || args.ga.meta == nullptr ||
        a.store == nullptr || a.max_bits == nullptr || args.cand == nullptr || args.exact == nullptr || args.ctl == nullptr)
        return hipErrorInvalidValue;
    const int grid = mirror8_dims_grid(a.n_rows, a.dims, grid_cap);
    bool masked = false;
    for (int i = 0; i < nq; ++i) {
        const MirrorMember& m = args.ga.g.m[i];
        if (m.k < 1 || m.k > MIRROR8_MAX_K || m.kpad < m.k || m.query == nullptr || m.partials == nullptr || m.hits == nullptr || m.certified == nullptr ||
            m.partials != args.ga.g.m[0].partials + (size_t)i * grid * MIRROR_KP)       // the selection takes the members' lists back to back
            return hipErrorInvalidValue;
        masked = masked || m.bitmap != nullptr;
    }
    return with_scan_shape(Mirror8WideDims{}, a.dims, [&](auto s) {
        return with_metric_in<M_COS, M_DOT>(metric, [&](auto mt) {
            constexpr int D = decltype(s)::DIMS, M = decltype(mt)::value;
            Mirror8DimsArgs d = args;
            d.ga.g.a.lists = grid;
            if (masked) launch_pass8<D, M, true>(d.ga, nq, grid, st);
            else launch_pass8<D, M, false>(d.ga, nq, grid, st);
            hipError_t err = hipGetLastError();
            if (err != hipSuccess) return err;
            err = launch_mirror_wide_select(d.ga.g.m[0].partials, grid, MIRROR8_DIMS_C, d.cand, d.ctl, st, nq);
            if (err != hipSuccess) return err;
            hipLaunchKernelGGL((mirror8_dims_rescore_kernel<D, M>), dim3(MIRROR8_DIMS_C / Rescore8Shape<D>::ROWS_PER_BLOCK, nq), dim3(SCAN_THREADS), 0, st, d);
            if ((err = hipGetLastError()) != hipSuccess) return err;
            hipLaunchKernelGGL((mirror8_dims_finish_kernel<D, M>), dim3(nq), dim3(MERGE_THREADS), 0, st, d);
            return hipGetLastError();
        }, hipErrorInvalidValue);
    }, hipErrorInvalidValue);
}

}  // namespace wax
