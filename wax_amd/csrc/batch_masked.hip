// batch_masked.hip — a batch of queries under ONE row predicate: one bf16 MFMA pass over the mirror under the predicate's row bitmap,
// then one finish workgroup per query ("The masked batch pass"; wax_hip_search_batch_masked, api_batch_masked.inc).
//
//   batch_masked_kernel<D, METRIC>   grid (row shares, blocks of 256 queries), 8 waves. Wave w keeps its 32 queries x D as bf16 MFMA
//                                    fragments in registers for the whole launch (the prep kernel's fragment-ordered copy, GemmArgs::qf).
//                                    The workgroup walks its contiguous share of the 32-row tiles; a tile whose bitmap word is zero is
//                                    neither loaded nor scored. A live tile is staged in LDS in chunks of 32 rows x 384 columns (one buffer;
//                                    the next chunk's loads are in flight in registers under the products) and read by all eight waves.
//                                    v_mfma_f32_32x32x16_bf16 takes the TILE fragment first and the QUERY fragment second, so a lane's 16
//                                    accumulators are 16 rows of ONE query (lane & 31): the selection is lane-local — the row's bitmap
//                                    bit, then one compare against the lane's running bound. Survivors go to the lane's own list in LDS
//                                    (BM_CAP keys); a list that cannot take a tile's survivors is rank-sorted by the wave down to its BM_KEEP
//                                    best, whose last key is the new bound. No sampling launch and no global threshold: the bound warms up inside the share.
//                                    Published per (query, share): the two half-wave lists (disjoint rows of the same query, BM_KEEP keys
//                                    each) and per half the bound above which it dropped rows (KEY_PAD: it dropped none).
//   batch_masked_finish_kernel       one workgroup per query: the BM_CAND best listed keys (wave lists + rank merge, topk.h), re-scored
//                                    with row_distance against the f32 store (the bits of the single-query scan), sorted by (distance,
//                                    row), the k best with frame ids, and the certificate of DESIGN 4.4: a passing row that was not
//                                    re-scored has an approximate key >= a_max = min(dropped bounds, the merge's cut), so its exact
//                                    distance is >= dist(a_max) - eps, eps the prep kernel's measured two-operand bound. Certified when
//                                    that exceeds the exact k-th (strictly: ties stay uncertified) or when nothing was dropped at all.
//
// Every list, bound and counter is written with vector stores.
#include <type_traits>

#include "kernels.h"
#include "row_math.h"
#include "topk.h"

namespace wax {

typedef float bm_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bm_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int bm_u32x4 __attribute__((ext_vector_type(4)));

constexpr int BM_WAVES = 8, BM_THREADS = BM_WAVES * WAVE;
constexpr int BM_TILE = 32;                              // rows per tile = rows of one bitmap word
constexpr int BM_KC = 384;                               // columns per staged chunk (D = 384: one chunk per tile, 768: two)
constexpr int BM_ROWB = BM_KC * 2 + 16;                  // bytes per staged row: + 16 so that 16 rows' fragment reads cover all 64 banks
constexpr int BM_CHUNK_BYTES = BM_TILE * BM_ROWB;
constexpr int BM_PIECES = BM_TILE * BM_KC * 2 / 16 / BM_THREADS;   // 16-byte pieces of a chunk per thread (3)
constexpr int BM_KEEP = BM_LIST / 2, BM_CAP = BM_KEEP + 16;   // keys a prune keeps; slots of a lane's list: the 16 rows of a tile fit behind a prune
constexpr size_t BM_LDS_BYTES = (size_t)BM_CHUNK_BYTES + (size_t)BM_THREADS * BM_CAP * sizeof(int64_t);
static_assert(BM_PIECES * BM_THREADS * 16 == BM_TILE * BM_KC * 2 && BM_CAP <= 64 && BM_KEEP + 1 <= BM_CAP, "geometry");
static_assert(BM_LDS_BYTES <= 160 * 1024, "one workgroup per CU");

// One lane's list (n > BM_KEEP unique keys at `list`) -> its BM_KEEP smallest, ascending, in list[0 .. BM_KEEP); returns the last of them.
// The whole wave works on the one list: lane j < n holds key j and ranks it against the others by readlane (no LDS traffic between the
// load and the store; a call into wave_prune would spill the resident query fragments around it).
__device__ __forceinline__ int64_t bm_prune(int64_t* list, int n, int lane) {
    wave_lds_fence();
    const int64_t mine = lane < n ? list[lane] : KEY_PAD;
    int rank = 0;
#pragma unroll
    for (int o = 0; o < BM_CAP; ++o) rank += readlane_i64(mine, o) < mine ? 1 : 0;
    wave_lds_fence();
    if (lane < n && rank < BM_KEEP) list[rank] = mine;
    const unsigned long long last = __ballot(lane < n && rank == BM_KEEP - 1);
    wave_lds_fence();
    return readlane_i64(mine, (int)__builtin_ctzll(last));
}

template <int D, int METRIC>
__global__ __launch_bounds__(BM_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void batch_masked_kernel(BatchMaskedArgs a) {
    static_assert(D % BM_KC == 0 && D / BM_KC <= 2 && METRIC != M_L2, "one or two whole chunks; cosine / dot");
    constexpr int NCH = D / BM_KC, KS = BM_KC / 16, KST = D / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char bm_smem[];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    int64_t* const my_list = reinterpret_cast<int64_t*>(bm_smem + BM_CHUNK_BYTES) + (size_t)t * BM_CAP;
    int64_t* const wave_lists = my_list - (size_t)lane * BM_CAP;
    const uint32_t share = blockIdx.x, shares = gridDim.x, qblock = blockIdx.y;
    const uint32_t n_tiles = (a.n_rows + BM_TILE - 1) / BM_TILE;
    const uint32_t t_begin = (uint32_t)((uint64_t)n_tiles * share / shares), t_end = (uint32_t)((uint64_t)n_tiles * (share + 1) / shares);

    // this wave's 32 queries, resident: lane l holds query l & 31, elements 16 ks + 8 (l >> 5) .. + 7 of every k-step
    bm_bf16x8 bq[KST];
    {
        const bm_u32x4* qf = reinterpret_cast<const bm_u32x4*>(a.qf) + ((size_t)(qblock * BM_WAVES + wave) * KST) * 64 + lane;
#pragma unroll
        for (int ks = 0; ks < KST; ++ks) bq[ks] = __builtin_bit_cast(bm_bf16x8, qf[(size_t)ks * 64]);
    }

    // the next tile at or after `from` with a passing row (t_end: none); every wave walks the same words
    uint32_t skipped = 0, word = 0;
    auto next_live = [&](uint32_t from) -> uint32_t {
        for (; from < t_end; ++from) {
            word = a.bitmap[__builtin_amdgcn_readfirstlane(from)];
            if (word != 0u) break;
            ++skipped;
        }
        return from;
    };
    const unsigned char* const mirror = reinterpret_cast<const unsigned char*>(a.mirror);
    bm_u32x4 stage[BM_PIECES];
    auto fetch = [&](uint32_t tile, int ch) {
#pragma unroll
        for (int p = 0; p < BM_PIECES; ++p) {
            const int piece = t + p * BM_THREADS, row = piece / (BM_KC / 8), c16 = piece % (BM_KC / 8);
            stage[p] = *reinterpret_cast<const bm_u32x4*>(mirror + ((size_t)(tile * BM_TILE + row) * D + (size_t)ch * BM_KC) * 2 + (size_t)c16 * 16);
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int p = 0; p < BM_PIECES; ++p) {
            const int piece = t + p * BM_THREADS, row = piece / (BM_KC / 8), c16 = piece % (BM_KC / 8);
            *reinterpret_cast<bm_u32x4*>(bm_smem + row * BM_ROWB + c16 * 16) = stage[p];
        }
    };

    int cnt = 0;
    int64_t bound = KEY_PAD;                             // only keys below it can still enter; KEY_PAD until the first prune: nothing dropped
    const uint32_t half_row = 4u * ((uint32_t)lane >> 5);
    auto prune_lanes = [&](unsigned long long who) {     // (wave-uniform mask; every lane in it holds more than BM_KEEP keys)
        while (who != 0ull) {
            const int owner = (int)__builtin_ctzll(who);
            who &= who - 1ull;
            const int64_t tau = bm_prune(wave_lists + (size_t)owner * BM_CAP, __builtin_amdgcn_readlane(cnt, owner), lane);
            if (lane == owner) { bound = tau; cnt = BM_KEEP; }
        }
    };
    uint32_t tile = next_live(t_begin), tile_word = word;
    int ch = 0;
    if (tile < t_end) { fetch(tile, 0); put(); }
    __syncthreads();
    bm_f32x16 acc = {};
    const unsigned char* const frag = bm_smem + (lane & 31) * BM_ROWB + (lane >> 5) * 16;
    while (tile < t_end) {                                // (workgroup-uniform)
        uint32_t ntile = tile, nword = tile_word;
        int nch = ch + 1;
        if (nch == NCH) { nch = 0; ntile = next_live(tile + 1); nword = word; }
        const bool more = ntile < t_end;
        if (more) fetch(ntile, nch);                      // in flight under the products and the selection
        auto mfma_chunk = [&](auto c) {                    // (the chunk is a constant: bq stays in registers)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const bm_bf16x8 fa = __builtin_bit_cast(bm_bf16x8, *reinterpret_cast<const bm_u32x4*>(frag + ks * 32));
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, bq[decltype(c)::value * KS + ks], acc, 0, 0, 0);
                if ((ks & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // four fragments in flight, not all of them: 768-d has no registers to spare
            }
        };
        if (NCH == 1 || ch == 0) mfma_chunk(std::integral_constant<int, 0>{});
        else mfma_chunk(std::integral_constant<int, NCH - 1>{});
        if (ch == NCH - 1) {
            // lane-local selection: acc[i] is row (i & 3) + 8 (i >> 2) + 4 (lane >> 5) of the tile against query lane & 31
            const uint32_t row0 = a.row_base + tile * BM_TILE;
            auto key_of = [&](int i, uint32_t r) {
                float d = 1.0f - acc[i];                  // cosine (rows and queries normalised) and dot alike
                d = (d != d) ? __builtin_inff() : d;
                return make_key(d + 0.0f, row0 + r);
            };
            int n_pass = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t r = (uint32_t)((i & 3) + 8 * (i >> 2)) + half_row;
                n_pass += (((tile_word >> r) & 1u) != 0u && key_of(i, r) < bound) ? 1 : 0;
            }
            // a lane whose survivors do not fit is pruned first: BM_KEEP keys stay, so the 16 rows of a tile always fit behind it
            prune_lanes(__ballot(cnt + n_pass > BM_CAP));
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t r = (uint32_t)((i & 3) + 8 * (i >> 2)) + half_row;
                const int64_t key = key_of(i, r);
                if (((tile_word >> r) & 1u) != 0u && key < bound) my_list[cnt++] = key;
            }
            acc = bm_f32x16{};
        }
        __syncthreads();                                  // every wave has read the chunk
        if (more) put();
        __syncthreads();
        tile = ntile; tile_word = nword; ch = nch;
    }

    // the end of the share: every lane's list down to BM_KEEP keys, then the two half-wave lists of a query side by side
    prune_lanes(__ballot(cnt > BM_KEEP));
    const uint32_t q = qblock * BM_QUERIES + (uint32_t)wave * 32u + ((uint32_t)lane & 31u);
    const uint32_t halfw = (uint32_t)lane >> 5;
    int64_t* out = a.lists + ((size_t)q * shares + share) * BM_LIST + halfw * BM_KEEP;
#pragma unroll
    for (int i = 0; i < BM_KEEP; ++i) out[i] = i < cnt ? my_list[i] : KEY_PAD;
    a.bounds[((size_t)q * shares + share) * 2 + halfw] = bound;
    if (t == 0) a.skipped[qblock * shares + share] = skipped;
}

// ---- the finish: one workgroup per query -----------------------------------------------------------------------------------------
template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS) void batch_masked_finish_kernel(BatchMaskedFinishArgs a) {
    constexpr int D4 = ScanShape<DIMS>::D4, GROUP = ScanShape<DIMS>::GROUP, LOADS = ScanShape<DIMS>::LOADS;
    constexpr int RPW = WAVE / GROUP, ROWS_PER_PASS = RPW * SCAN_WAVES, PASSES = BM_CAND / ROWS_PER_PASS, WCAP = 256;
    static_assert(BM_CAND % ROWS_PER_PASS == 0 && WCAP - 64 >= BM_CAND && BM_CAND <= SCAN_THREADS, "whole passes; a push fits behind a prune");
    __shared__ int64_t wbuf[SCAN_WAVES][WCAP], approx[BM_CAND], exact[BM_CAND], sorted[BM_CAND];
    __shared__ long long bound_min;
    __shared__ int wcount[SCAN_WAVES], n_listed;
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t q = blockIdx.x;
    const uint32_t n_keys = a.shares * BM_LIST;
    const int64_t* keys = a.lists + (size_t)q * n_keys;
    if (t == 0) { bound_min = KEY_PAD; n_listed = 0; }
    __syncthreads();

    // (1) the BM_CAND best listed keys -> approx[] (KEY_PAD behind them), the smallest dropped bound, how many keys were listed
    {
        int64_t b = KEY_PAD;
        for (uint32_t i = t; i < a.shares * 2u; i += SCAN_THREADS) { const int64_t v = a.bounds[(size_t)q * a.shares * 2u + i]; b = v < b ? v : b; }
        if (b != KEY_PAD) atomicMin(&bound_min, (long long)b);
    }
    if (n_keys <= (uint32_t)BM_CAND) {
        if (t < BM_CAND) approx[t] = (uint32_t)t < n_keys ? keys[t] : KEY_PAD;
    } else {
        WaveTopK<WCAP> tk;
        tk.init(wbuf[wave], BM_CAND);
        int mine = 0;
        for (uint32_t i0 = (uint32_t)wave * 64u; i0 < n_keys; i0 += SCAN_THREADS) {   // (wave-uniform trip count)
            const uint32_t i = i0 + (uint32_t)lane;
            const int64_t key = i < n_keys ? keys[i] : KEY_PAD;
            mine += key != KEY_PAD ? 1 : 0;
            tk.make_room(64);
            tk.push(key, key != KEY_PAD);
        }
        tk.finalize();
        if (lane == 0) wcount[wave] = tk.cnt;
        if (mine) atomicAdd(&n_listed, mine);
        __syncthreads();
        block_rank_merge<SCAN_WAVES>(&wbuf[0][0], WCAP, wcount, BM_CAND, approx);
    }
    __syncthreads();
    const bool cut = n_keys > (uint32_t)BM_CAND && n_listed > BM_CAND;   // the merge dropped listed keys: all of them above approx[BM_CAND - 1]

    // (2) exact f32 re-score: row_distance at the f32 scan's shape for this dimension
    const float q_norm = a.q_norm[q];
    const int sub = lane / GROUP, gl = lane % GROUP;
    const f32x4* q4 = reinterpret_cast<const f32x4*>(a.queries + (size_t)q * DIMS);
    f32x4 qv[LOADS];
#pragma unroll
    for (int j = 0; j < LOADS; ++j) qv[j] = q4[gl + j * GROUP];
    const f32x4* __restrict__ store4 = reinterpret_cast<const f32x4*>(a.store);
#pragma unroll 2
    for (int p = 0; p < PASSES; ++p) {
        const int i = p * ROWS_PER_PASS + wave * RPW + sub;
        const int64_t key = approx[i];
        const uint32_t grow = key_row(key), lrow = grow - a.row_base;
        const bool live = key != KEY_PAD && lrow < a.n_rows;
        const f32x4* src = store4 + (size_t)(live ? lrow : 0u) * D4 + gl;
        f32x4 v[LOADS];
#pragma unroll
        for (int j = 0; j < LOADS; ++j) v[j] = src[j * GROUP];
        const float d = row_distance<GROUP, LOADS, METRIC>(qv, v, q_norm);
        if (gl == GROUP - 1) exact[i] = live ? make_key(d, grow) : KEY_PAD;
    }
    __syncthreads();

    // (3) rank sort of the exact keys (unique rows; KEY_PAD ties broken by position)
    if (t < BM_CAND) {
        const int64_t key = exact[t];
        int rank = 0;
        for (int j = 0; j < BM_CAND; ++j) {
            const int64_t o = exact[j];
            rank += (o < key || (o == key && j < t)) ? 1 : 0;
        }
        sorted[rank] = key;
    }
    __syncthreads();

    // (4) the k best with frame ids
    for (int i = t; i < a.k; i += SCAN_THREADS) {
        wax_hip_hit h;
        h.key = sorted[i];
        h.frame_id = ID_PAD;
        if (h.key != KEY_PAD) {
            const uint32_t local = key_row(h.key) - a.row_base;
            h.frame_id = (a.ids != nullptr && local < a.n_rows) ? a.ids[local] : (uint64_t)key_row(h.key);
        }
        a.hits[(size_t)q * a.k + i] = h;
    }
    // (5) the certificate
    if (t == 0) {
        int64_t a_max = (int64_t)bound_min;
        if (cut && approx[BM_CAND - 1] < a_max) a_max = approx[BM_CAND - 1];
        bool ok = a_max == KEY_PAD;                        // nothing dropped anywhere: every passing row was re-scored
        if (!ok) {
            const float eps = a.eps[q];
            const int64_t kth = sorted[a.k - 1];
            const float da = key_distance(a_max), dk = key_distance(kth);
            ok = kth != KEY_PAD && __builtin_isfinite(da) && __builtin_isfinite(dk) && __builtin_isfinite(eps) && q_norm == q_norm &&
                 (da - eps > dk);                          // strict: ties stay uncertified
        }
        a.certified[q] = ok ? 1u : 0u;
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------------
bool batch_masked_dims(uint32_t dims, int metric) { return (dims == 384u || dims == 768u) && (metric == M_COS || metric == M_DOT); }

template <int D, int METRIC>
static hipError_t launch_bm_pass(const BatchMaskedArgs& a, hipStream_t st) {
    static std::atomic<uint64_t> configured{0};
    const hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&batch_masked_kernel<D, METRIC>), BM_LDS_BYTES, configured);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((batch_masked_kernel<D, METRIC>), dim3(a.shares, a.nq_pad / BM_QUERIES), dim3(BM_THREADS), BM_LDS_BYTES, st, a);
    return hipGetLastError();
}

hipError_t launch_batch_masked(const BatchMaskedArgs& a, int metric, hipStream_t st) {
    const uint32_t n_tiles = (a.n_rows + BM_TILE - 1) / BM_TILE;
    if (!batch_masked_dims(a.dims, metric) || a.n_rows < 1 || a.nq_pad < BM_QUERIES || a.nq_pad % BM_QUERIES != 0 || a.shares < 1 || a.shares > n_tiles ||
        !a.mirror || !a.qf || !a.bitmap || !a.lists || !a.bounds || !a.skipped)
        return hipErrorInvalidValue;
    if (a.dims == 384u) return metric == M_COS ? launch_bm_pass<384, M_COS>(a, st) : launch_bm_pass<384, M_DOT>(a, st);
    return metric == M_COS ? launch_bm_pass<768, M_COS>(a, st) : launch_bm_pass<768, M_DOT>(a, st);
}

hipError_t launch_batch_masked_finish(const BatchMaskedFinishArgs& a, int metric, hipStream_t st) {
    if (!batch_masked_dims(a.dims, metric) || a.nq < 1 || a.k < 1 || a.k > BM_MAX_K || a.shares < 1 || !a.lists || !a.bounds || !a.store || !a.queries ||
        !a.q_norm || !a.eps || !a.hits || !a.certified)
        return hipErrorInvalidValue;
    if (a.dims == 384u) {
        if (metric == M_COS) hipLaunchKernelGGL((batch_masked_finish_kernel<384, M_COS>), dim3(a.nq), dim3(SCAN_THREADS), 0, st, a);
        else hipLaunchKernelGGL((batch_masked_finish_kernel<384, M_DOT>), dim3(a.nq), dim3(SCAN_THREADS), 0, st, a);
    } else {
        if (metric == M_COS) hipLaunchKernelGGL((batch_masked_finish_kernel<768, M_COS>), dim3(a.nq), dim3(SCAN_THREADS), 0, st, a);
        else hipLaunchKernelGGL((batch_masked_finish_kernel<768, M_DOT>), dim3(a.nq), dim3(SCAN_THREADS), 0, st, a);
    }
    return hipGetLastError();
}

}  // namespace wax
