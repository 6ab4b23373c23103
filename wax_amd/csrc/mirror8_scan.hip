// mirror8_scan.hip — one query (or up to four) against the 8-bit code mirror of the store, answered in f32 ("Eight bits
// per element").
//
// mirror_scan.hip's pass runs at the HBM read rate, so the next factor is again bytes per pass: one byte per element plus 8 bytes per
// row instead of two bytes per element. The pass has mirror_pass's frame (mirror_pass.h: persistent grid, one WaveTopK list per wave
// and query, the workgroup rank merge, MIRROR_KP keys per workgroup and query, the clamp of tail rows) and mirror_finish
// (mirror_finish.h) for the exact re-score, but the sums run on the matrix pipe — code8_pass below — with another certificate:
//   the row       D bytes: code_i + 128, code_i = rint(x^_i / scale) in [-127, 127], scale = max|x^| / 127 of THAT row (x^: the f32 row,
//                 normalised for cosine as mirror_kernel does). One v_xor per dword takes the bias off.
//   the query     three int8 digits per element (QueryPlanes): q^_i = delta * m_i, m_i = 16384 a_i + 128 b_i + c_i, so that
//                 sum_i m_i code_i is three exact integer dots — one v_mfma_i32_16x16x64_i8 column each.
//   the key       meta[row] = {scale, err}, err >= ||scale * code - x^||_2 (measured per row by mirror8_kernel, rounded up). With
//                 s = delta * scale * sum_i m_i code_i:  |s - q.x^| <= ||q|| err (up to the slack below), so
//                     cosine  lb = 1 - s / ||q|| - err          dot  lb = 1 - s - ||q|| err
//                 is a LOWER BOUND of the row's distance. A NaN lb, and err = +inf, give -inf: such a row is always a candidate and
//                 is re-scored exactly.
//   certificate   lb_KP - slack > d_k, strict. Every row outside the candidates has lb >= lb_KP, hence an exact distance
//                 >= lb_KP - slack > d_k. slack (Mirror8Slack) holds what err does not — see there.
#include <cstring>

#include "mirror8_layout.h"
#include "mirror_finish.h"
#include "mirror_pass.h"

namespace wax {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// the wave's maximum in every lane (the build kernel and the query's quantiser)
__device__ inline float wave_max64(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// A 16-row tile is one MFMA operand A: lane l holds 16 codes of row (l & 15) per k-step, bytes [64 s + 16 (l >> 4), + 16) of the row at
// step s — the sum over k does not care which 16 elements a lane holds as long as operand B holds the same ones. The buffer is stored
// in that order (mirror8_layout.h), so load s of a wave is 1024 contiguous bytes of the tile.
// How a pass reads its tiles — the kernels below all run Code8Shipped; tools/code8_shape_probe.hip times the others on the same body:
//   TILED   the buffer is in mirror8_layout.h's order; else row-major ([row][element]: an instruction touches sixteen 64-byte
//           halves of lines, and every line must stay in the vector L1 between the two instructions that read it)
//   NT      non-temporal code loads
//   TILES   tiles per wave iteration, all loaded before the first product
//   AHEAD   the wave's first iteration is loaded in front of the query prologue (query_delta, query_digits: about a thousand
//           instructions that depend on no row), which then runs under the first miss
template <bool TILED_, bool NT_, int TILES_, bool AHEAD_>
struct Code8Loads {
    static constexpr bool TILED = TILED_, NT = NT_, AHEAD = AHEAD_;
    static constexpr int TILES = TILES_;
    static_assert(TILES >= 1 && TILES <= 2, "tiles per wave iteration");
    static __host__ __device__ constexpr size_t offset(uint64_t row, uint32_t element, uint32_t dims) {
        return TILED ? mirror8_offset(row, element, dims) : (size_t)row * dims + element;
    }
};
// What profiles/r26/a_code8_shape_probe.jsonl chose (10M x 384, lone / four queries, ms): row-major plain 0.627 / 0.679 and non-temporal
// 0.669 / 0.731; tiled plain 0.632 / 0.682, tiled non-temporal 0.570 / 0.625. Whole lines that nothing reads twice need no place
// in the cache. Two tiles per iteration change neither form by more than the spread (0.572 / 0.625), and neither does AHEAD
// (0.570 / 0.625) — which keeps the tile's registers live across the prologue: 26 VGPRs more, three waves per SIMD instead of four
// at 384-d and spills at 768-d. Not shipped.
using Code8Shipped = Code8Loads<true, true, 1, false>;

template <int DIMS, class LOADS = Code8Shipped>
struct Code8Tiles {
    static constexpr int TILE = 16;                    // rows per MFMA; one make_room takes an iteration's
    static constexpr int KSTEPS = DIMS / 64;           // MFMAs (and dwordx4 loads per lane) per tile: 96 B in flight per lane at 384-d
    static constexpr int RPC = TILE * LOADS::TILES;    // rows per wave iteration
    static_assert(DIMS % 64 == 0, "whole k-steps");
    static_assert(TILE == (int)MIRROR8_TILE_ROWS, "the layout's tile is the operand's");
};

// The query as three balanced base-128 digits per element, exact by construction:
//   M = 63 * 16384 + 63 * 128 + 63, delta = max|q| / M, m_i = rint(q_i * (1 / delta)) clamped to [-M, M] (one division per wave, one
//   product per element: both rounded, 2^-23 |m_i| <= 1/8 between them), m_i = 16384 a_i + 128 b_i + c_i with every digit in
//   [-64, 63], so ||q^ - q|| <= delta sqrt(D) (1/2 + 1/8) <= 1.18e-5 ||q|| at 384-d whatever the elements; tests/mirror8_planes_ref.py
//   restates it and tests/test_mirror8_planes_cpu.py finds 5.7e-6 at most, inside delta sqrt(D) / 2 every time.
// A query with a non-finite element gets delta = NaN: every s is NaN, every key -inf, the 64th key is not finite and the finish
// refuses the certificate. The all-zero query — and one whose delta would be subnormal, max|q| < 1.3e-32, where 1 / delta leaves
// the f32 range — gets delta = 0 and digits 0 (s = 0, like the f32 sum to within 1e-30 ||v||).
constexpr int PLANE_M = 63 * 16384 + 63 * 128 + 63;

// delta of the query at q4: the whole wave reads it once
template <int DIMS>
__device__ __forceinline__ float query_delta(const f32x4* q4, int lane) {
    float amax = 0.f;
    bool bad = false;
#pragma unroll
    for (int c = 0; c < (DIMS / 4 + WAVE - 1) / WAVE; ++c) {
        const int idx = lane + c * WAVE;
        if (idx < DIMS / 4) {
            const f32x4 v = q4[idx];
            bad = bad || !__builtin_isfinite(v.x) || !__builtin_isfinite(v.y) || !__builtin_isfinite(v.z) || !__builtin_isfinite(v.w);
            amax = fmaxf(fmaxf(amax, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        }
    }
    amax = wave_max64(amax);
    const float delta = __fdiv_rn(amax, (float)PLANE_M);
    return __ballot(bad) != 0ull ? __builtin_nanf("") : delta >= 1.17549435e-38f ? delta : 0.f;
}

// digit `plane` (0: a, 1: b, 2: c, else 0) of the 16 elements at q, as the bytes of one MFMA operand
__device__ __forceinline__ i32x4 query_digits(const float* q, float inv_delta, int plane) {
    const f32x4* q4 = reinterpret_cast<const f32x4*>(q);
    i32x4 out;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const f32x4 v = q4[w];
        const float x[4] = {v.x, v.y, v.z, v.w};
        unsigned int word = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float t = x[j] * inv_delta;
            t = rintf(fminf(fmaxf(t, -(float)PLANE_M), (float)PLANE_M));
            const int m = (int)t;
            const int c = ((m + 64) & 127) - 64, m1 = (m - c) >> 7;
            const int b = ((m1 + 64) & 127) - 64, a = (m1 - b) >> 7;
            const int d = plane == 0 ? a : plane == 1 ? b : plane == 2 ? c : 0;
            word |= ((unsigned int)d & 0xffu) << (8 * j);
        }
        out[w] = (int)word;
    }
    return out;
}

// v's value in lane Q of every quad
template <int Q>
__device__ __forceinline__ float quad_bcast(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), Q * 0x55, 0xF, 0xF, true));
}

// The key of one row for one query, from the integer sum S = sum_i m_i code_i (as a float: exact or rounded by code8_sum), delta,
// the row's {scale, err} and the query's norm: the ONE float epilogue of every form of the pass.
template <int METRIC>
__device__ __forceinline__ float code8_key(float S, float delta, f32x2 meta, float inv_qn, float q_norm) {
    const float s = (delta * meta.x) * S;
    const float lb = METRIC == M_COS ? (1.0f - s * inv_qn) - meta.y : (1.0f - s) - q_norm * meta.y;
    return (lb != lb) ? -__builtin_inff() : lb;
}

// S from the three plane sums (each below 2^24 in magnitude: the conversions are exact); two roundings
__device__ __forceinline__ float code8_sum(float pa, float pb, float pc) {
    return __builtin_fmaf(16384.0f, pa, __builtin_fmaf(128.0f, pb, pc));
}

// ONE pass of NQ queries over the code mirror on the matrix pipe: mirror_pass's sibling. Operand B's 16 columns are (query, plane):
// column 4 i + t holds digit plane t of query i (t = 3: zeros), for the whole launch, KSTEPS x 4 VGPRs whatever NQ. The accumulator of
// lane l holds rows 4 (l >> 4) + reg, reg = 0 .. 3, of column l & 15; the three planes of a query sit in one quad, so three quad
// broadcasts and two fma give every lane of the quad S of its query for the four rows, and lane t of the quad keeps row
// 4 (l >> 4) + t: the wave then holds the tile's 16 rows x 4 queries, one key per lane, and one push per query offers 16 rows.
// The integer sums are exact and the float epilogue is one function of (S, delta, meta, norm), so a row's key for a query is the same
// alone and in a pass of 2, 3 or 4. WRITE_KEYS (mirror8_keys_kernel, a diagnostic): every key is written to keys_out[row] and no
// list is kept.
// MASKED (the predicate tickets' pass): every member may carry a row bitmap (qs.bitmap(i); predicate.hip's: every word
// written, bits of rows >= n clear; null = every row may be offered). A tile's 16 bits are half a word — tile c is half c & 1 of
// word c >> 1 — and every lane reads the word of ITS query (one address per quad column group, the dead columns read 0), one
// iteration ahead like mirror_pass. A tile whose bits are zero for every live member is skipped before its loads and make_room (the
// ballot makes the test wave-uniform); otherwise a lane's key is offered only where bit 4 kg + plane of its own query is set. The
// sums and the epilogue do not see the bitmap: a row's key is what it is unmasked.
template <int DIMS, int METRIC, int NQ, bool WRITE_KEYS, bool MASKED, class QUERIES, class LOADS = Code8Shipped, class FRAME = FrameShipped>
__device__ __forceinline__ void code8_pass(const unsigned char* __restrict__ codes, const f32x2* __restrict__ sides, const MirrorScanArgs& a,
                                           const QUERIES& qs, float* __restrict__ keys_out, int64_t* lds) {
    using T = Code8Tiles<DIMS, LOADS>;
    constexpr int KSTEPS = T::KSTEPS, TILE = T::TILE, RPC = T::RPC, TILES = LOADS::TILES;
    static_assert(NQ >= 1 && NQ <= MIRROR_MAX_NQ && MIRROR_MAX_NQ * 4 <= 16, "four columns per query");
    static_assert(!MASKED || TILES == 1, "the skip test and the bitmap word are a tile's");

    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const int col = lane & 15, kg = lane >> 4;        // operand A: row col of the tile, bytes 16 kg of every 64; operand B: column col
    const int myq = col >> 2, plane = col & 3;        // the query and plane of this lane's column; after the combine: row 4 kg + plane
    const bool live = myq < NQ;
    const uint32_t n = a.n_rows;

    const uint32_t nchunks = (n + RPC - 1) / RPC;
    const uint32_t gwave = blockIdx.x * SCAN_WAVES + wave;
    const uint32_t nwaves = gridDim.x * SCAN_WAVES;

    PassLists<NQ, FRAME> lists;                         // (WRITE_KEYS keeps none)
    lists.clk.begin();
    if constexpr (!WRITE_KEYS) lists.init(lds, wave);

    // the codes of the iteration's tiles: every load is issued before the first product. The clamp makes tail lanes re-read the last
    // row (a tile past the last one, TILES > 1, reads it in every lane): no byte that the writer did not write reaches a key.
    u32x4 v[TILES][KSTEPS];
    auto load_tiles = [&](uint32_t chunk) {
#pragma unroll
        for (int u = 0; u < TILES; ++u) {
            const uint32_t ra = (chunk * TILES + u) * TILE + col;        // the row this lane loads codes of
            const uint32_t rc = ra < n ? ra : n - 1;
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s) {
                const u32x4* p = reinterpret_cast<const u32x4*>(codes + LOADS::offset(rc, 64 * s + 16 * kg, DIMS));
                v[u][s] = LOADS::NT ? __builtin_nontemporal_load(p) : *p;
            }
        }
    };
    if constexpr (LOADS::AHEAD) { if (gwave < nchunks) load_tiles(gwave); }

    // this lane's query: delta, the norm, and the digits of its plane at the lane's k-slices
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
    i32x4 b[KSTEPS];
    const float inv_delta = delta > 0.f ? __fdiv_rn(1.0f, delta) : 0.f;      // (delta = 0 or NaN: no digits)
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) b[s] = query_digits(mine + s * 64 + kg * 16, inv_delta, live ? plane : 3);

    // the word of this lane's query that holds tile c's bits (c < nchunks: row 16 c < n, so word c >> 1 exists)
    auto tile_word = [&](uint32_t c) -> uint32_t { return !live ? 0u : my_bitmap == nullptr ? 0xffffffffu : my_bitmap[c >> 1]; };
    uint32_t word = 0u, bits = 0xffffu;
    if constexpr (MASKED) word = gwave < nchunks ? tile_word(gwave) : 0u;   // one iteration ahead
    lists.clk.loop_begin();
    for (uint32_t chunk = gwave; chunk < nchunks; chunk += nwaves) {
        if constexpr (MASKED) {
            bits = (word >> ((chunk & 1u) * 16u)) & 0xffffu;
            const uint32_t next = chunk + nwaves;
            if (next < nchunks) word = tile_word(next);
            if (__ballot(bits != 0u) == 0ull) continue;          // wave-uniform: no member may be offered a row of the tile, so none is loaded
        }
        if (!LOADS::AHEAD || chunk != gwave) load_tiles(chunk);
        f32x2 side[TILES];
#pragma unroll
        for (int u = 0; u < TILES; ++u) {
            const uint32_t r = (chunk * TILES + u) * TILE + 4 * kg + plane;      // the row this lane will hold the key of
            side[u] = __builtin_nontemporal_load(sides + (r < n ? r : n - 1));
        }
        if constexpr (!WRITE_KEYS) lists.room(RPC);
#pragma unroll
        for (int u = 0; u < TILES; ++u) {
            const uint32_t r = (chunk * TILES + u) * TILE + 4 * kg + plane;
            i32x4 acc = {0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s) {
                const u32x4 x = v[u][s] ^ 0x80808080u;
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, x), b[s], acc, 0, 0, 0);
            }
            float S = 0.f;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const float pl = (float)acc[reg];
                const float Sr = code8_sum(quad_bcast<0>(pl), quad_bcast<1>(pl), quad_bcast<2>(pl));
                S = plane == reg ? Sr : S;
            }
            const float d = code8_key<METRIC>(S, delta, side[u], inv_qn, qn);
            bool offer = live && r < n;
            if constexpr (MASKED) offer = offer && ((bits >> (uint32_t)(4 * kg + plane)) & 1u) != 0u;
            if constexpr (WRITE_KEYS) {
                if (offer && myq == 0) keys_out[r] = d + 0.0f;
            } else {
                const int64_t key = make_key(d + 0.0f, a.row_base + r);
#pragma unroll
                for (int i = 0; i < NQ; ++i) lists.offer(i, key, offer && myq == i);
            }
        }
    }
    if constexpr (WRITE_KEYS) return;

    lists.finish(qs);
}

// launch(ScanShape<dims>, metric constant, grid) at the instantiation of (dims, metric), with the grid of code8_pass at that dimension
template <typename F>
inline hipError_t with_code8_pass(uint32_t n_rows, uint32_t dims, int metric, int grid_cap, F&& launch) {
    return with_scan_shape(MirrorDims{}, dims, [&](auto s) {
        return with_metric_in<M_COS, M_DOT>(metric, [&](auto m) {
            return launch(s, m, mirror_pass_grid(n_rows, Code8Tiles<decltype(s)::DIMS>::RPC, grid_cap));
        }, hipErrorInvalidValue);
    }, hipErrorInvalidValue);
}

// What the per-row err does not hold, as a bound on (lb as computed) - (the row's exact distance as row_distance computes it):
//  (a) the query's digits and the combine. s is delta * scale * S~ with S~ the twice-rounded 16384 P_a + 128 P_b + P_c (the plane
//      sums themselves are exact integers). With q^ = delta * m and x~ = scale * code:
//        - the query's rounding: |q^.x~ - q.x~| <= ||q^ - q|| ||x~|| <= (delta sqrt(D) / 2) (||x^|| + err), and delta = max|q| / M
//          <= ||q|| / 1 040 319, so at most 0.625 sqrt(D) / 1 040 319 ||q|| (||v|| + err) = 1.18e-5 ||q|| (||v|| + err) at 384-d
//          (err <= ||v||: < 2.4e-5 ||q|| ||v|| even for a row coded as badly as can be);
//        - the two fma roundings: each is relative 2^-24 of a partial sum, and by Cauchy-Schwarz delta scale |16384 P_a| (and the
//          smaller partial sums) <= ~||q^|| ||x~|| <= 1.01 ||q|| ||v||: < 4 u ||q|| ||v||.
//      Together < (1.25 sqrt(D) / 1 040 319 + 4 u) ||q|| ||v|| = 2.4e-5 (384-d), 3.4e-5 (768-d), below the
//      8192 u sqrt(D) / 127 ||q|| max||v|| = 7.5e-5 (384-d), 1.07e-4 (768-d) that this term has always been (it was sized for the f32
//      accumulation of the biased sum): both scale with sqrt(D), the factor of three between them holds at every D. The value stays;
//  (b) 3 D u ||q|| max||v|| for the f32 sums and normalisations on either side, as in the bf16 certificate;
//  (c) the roundings of delta * scale * S, / ||q||, the two subtractions, and the exact distance's own ~1e-6: 3e-6 (cosine),
//      3e-6 (1 + ||q|| max||v||) (dot) — a row that matters has |lb| <= 2 (1 + ||q|| max||v||).
// Cosine divides by ||q||, so both norms are 1 there.
struct Mirror8Slack {
    template <int DIMS, int METRIC>
    static __device__ __forceinline__ float eps(const MirrorScanArgs& a) {
        const double qn = METRIC == M_COS ? 1.0 + 1e-6 : (double)a.q_norm;
        const double vn = METRIC == M_COS ? 1.0 + 1e-6 : (double)__uint_as_float(a.max_bits[0]);
        const double u = 5.97e-8;
        const double acc = 8192.0 * u * __builtin_sqrt((double)DIMS) / 127.0;
        const double both = (acc + 3.0 * (double)DIMS * u) * qn * vn * 1.001;
        const float s = METRIC == M_COS ? (float)(both + 3e-6) : (float)(both + 3e-6 * (1.0 + qn * vn));
        return nextafterf(s, __builtin_inff());
    }
};

}  // namespace

template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS, 2) void mirror8_scan_kernel(Mirror8ScanArgsQ<DIMS> aq) {
    __shared__ int64_t lds[MIRROR_PASS_LDS];
    code8_pass<DIMS, METRIC, 1, false, false>(aq.codes, reinterpret_cast<const f32x2*>(aq.meta), aq.a, LoneQuery<Mirror8ScanArgsQ<DIMS>>{aq.a}, nullptr, lds);
}

template <int DIMS, int METRIC, int NQ>
__global__ __launch_bounds__(SCAN_THREADS, 2) void mirror8_scan_group_kernel(Mirror8GroupArgs ga) {
    static_assert(NQ >= 2, "a lone query has mirror8_scan_kernel");
    __shared__ int64_t lds[NQ * MIRROR_PASS_LDS];
    code8_pass<DIMS, METRIC, NQ, false, false>(ga.codes, reinterpret_cast<const f32x2*>(ga.meta), ga.g.a, MemberQueries{ga.g.m}, nullptr, lds);
}

// the pass of 1 .. 4 members of which at least one carries a row bitmap (MirrorMember::bitmap): the predicate tickets' pass
template <int DIMS, int METRIC, int NQ>
__global__ __launch_bounds__(SCAN_THREADS, 2) void mirror8_scan_masked_group_kernel(Mirror8GroupArgs ga) {
    __shared__ int64_t lds[NQ * MIRROR_PASS_LDS];
    code8_pass<DIMS, METRIC, NQ, false, true>(ga.codes, reinterpret_cast<const f32x2*>(ga.meta), ga.g.a, MemberQueries{ga.g.m}, nullptr, lds);
}

// the lone pass's keys, every row's (wax_hip_mirror8_keys: a diagnostic)
template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS, 2) void mirror8_keys_kernel(Mirror8ScanArgsQ<DIMS> aq, float* keys_out) {
    code8_pass<DIMS, METRIC, 1, true, false>(aq.codes, reinterpret_cast<const f32x2*>(aq.meta), aq.a, LoneQuery<Mirror8ScanArgsQ<DIMS>>{aq.a}, keys_out, nullptr);
}

// the frame alone on made-up keys (wax_hip_mirror_lists_probe: a diagnostic): code8_pass's walk and its lane-to-(query, row) map,
// with keys[q][slot] where the pass computes a key and KEY_PAD where it offers none
struct ProbePartials {
    int64_t* out;
    __device__ __forceinline__ int64_t* partials(int i) const { return out + (size_t)i * gridDim.x * MIRROR_KP; }
};
template <int NQ>
__global__ __launch_bounds__(SCAN_THREADS, 2) void mirror_lists_probe_kernel(const int64_t* __restrict__ keys, uint32_t n_slots, int64_t* __restrict__ out) {
    __shared__ int64_t lds[NQ * MIRROR_PASS_LDS];
    constexpr int TILE = 16;
    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const int myq = (lane & 15) >> 2, row = 4 * (lane >> 4) + (lane & 3);
    const uint32_t nchunks = (n_slots + TILE - 1) / TILE;
    PassLists<NQ> lists;
    lists.init(lds, wave);
    for (uint32_t chunk = blockIdx.x * SCAN_WAVES + wave; chunk < nchunks; chunk += gridDim.x * SCAN_WAVES) {
        const uint32_t slot = chunk * TILE + row;
        const int64_t key = (myq < NQ && slot < n_slots) ? keys[(size_t)myq * n_slots + slot] : KEY_PAD;
        lists.room(TILE);
#pragma unroll
        for (int i = 0; i < NQ; ++i) lists.offer(i, key, key != KEY_PAD && myq == i);
    }
    lists.finish(ProbePartials{out});
}

template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS) void mirror8_finish_kernel(Mirror8ScanArgsQ<DIMS> aq) {
    mirror_finish<DIMS, METRIC, Mirror8Slack>(aq.a, LoneQuery<Mirror8ScanArgsQ<DIMS>>::kernarg_floats());
}

// one workgroup per member
template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS) void mirror8_finish_group_kernel(Mirror8GroupArgs ga) {
    const MirrorMember& m = ga.g.m[blockIdx.x];
    mirror_finish<DIMS, METRIC, Mirror8Slack>(member_args(ga.g.a, m), reinterpret_cast<const f32x4*>(m.query));
}

// ---------------------------------------------------------------------------
// f32 rows -> biased codes + {scale, err}. One wave per row (mirror8_code_row), a tile per workgroup and four steps (mirror8_kernel). The f32 STORE is read, never the bf16 mirror (the errors would add).
//   x^      cosine: v * (1 / sqrt(m)), m = the scan's own sum of squares (scan_order_norm2), a row the scan scores 0 (sqrt(m) <= 1e-6,
//           NaN) becomes zero — mirror_kernel's rule and expression; dot: v.
//   scale   max|x^| / 127; code = rint(x^ / scale) clamped to +-127 (a zero row: scale 0, codes 0).
//   err     sqrt(sum_i fma(scale, code_i, -x^_i)^2): each difference is rounded once (relative 2^-24), the sum of D squares and the root
//           lose at most (D / 2 + 2) 2^-24 relative, so err * (1 + D 2^-23), then nextafter, is an upper bound. The differences are
//           squared and summed in units of 2^ex, scale = f * 2^ex (ldexpf: exact), and the root is scaled back: for a row of ordinary
//           magnitude that changes no bit, and a row of 1e-30 or 1e+21 — whose squared differences are 0 or +inf in f32 — gets the err
//           it has instead of 2^-149 (no bound at all) or +inf.
//   A row with an inf / NaN element (or whose scale or err is still not finite) gets err = +inf and scale 0.
// one row by one wave: its codes into the buffer at `codes` where mirror8_offset has row r, {scale, err} to meta_row; returns sqrt(m)
__device__ __forceinline__ float mirror8_code_row(const float* __restrict__ row, uint32_t dims, int normalize, int lane,
                                                  unsigned char* __restrict__ codes, uint32_t r, float* __restrict__ meta_row) {
    const uint32_t d4 = dims >> 2;
    const f32x4* row4 = reinterpret_cast<const f32x4*>(row);
    const float m = normalize == 16 ? scan_order_norm2<16>(row, dims, lane)
                  : normalize == 32 ? scan_order_norm2<32>(row, dims, lane) : scan_order_norm2<64>(row, dims, lane);
    const float n = sqrtf(m);
    const bool zero_row = normalize && !(n > COS_NORM_FLOOR);
    const float inv = normalize ? 1.0f / n : 1.0f;
    float amax = 0.f;
    bool bad = false;
    for (uint32_t c = lane; c < d4; c += WAVE) {
        const f32x4 v = row4[c];
        const float x[4] = {zero_row ? 0.f : v.x * inv, zero_row ? 0.f : v.y * inv, zero_row ? 0.f : v.z * inv, zero_row ? 0.f : v.w * inv};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bad = bad || !__builtin_isfinite(x[i]);
            amax = fmaxf(amax, fabsf(x[i]));
        }
    }
    amax = wave_max64(amax);
    bad = __ballot(bad) != 0ull;
    float scale = amax / 127.0f;
    if (!__builtin_isfinite(scale)) { bad = true; scale = 0.f; }
    int ex = 0;                              // scale = f * 2^ex, f in [0.5, 1): the differences are squared in units of 2^ex
    (void)frexpf(scale, &ex);
    float e2 = 0.f;
    for (uint32_t c = lane; c < d4; c += WAVE) {
        const f32x4 v = row4[c];
        const float x[4] = {zero_row ? 0.f : v.x * inv, zero_row ? 0.f : v.y * inv, zero_row ? 0.f : v.z * inv, zero_row ? 0.f : v.w * inv};
        unsigned int word = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float t = (scale > 0.f && x[i] == x[i]) ? x[i] / scale : 0.f;
            t = rintf(fminf(fmaxf(t, -127.0f), 127.0f));
            const float d = ldexpf(fmaf(scale, t, -x[i]), -ex);
            e2 = fmaf(d, d, e2);
            word |= (unsigned int)((int)t + 128) << (8 * i);
        }
        *reinterpret_cast<unsigned int*>(codes + mirror8_offset(r, 4 * c, dims)) = word;
    }
    e2 = group_sum<64>(e2);
    e2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e2), 63));
    float errn = sqrtf(e2) * (1.0f + (float)dims * 1.1920929e-7f);
    errn = nextafterf(errn, __builtin_inff());
    float err = ldexpf(errn, ex);
    if (ldexpf(err, -ex) < errn) err = nextafterf(err, __builtin_inff());     // back in the subnormal range: rounded up, never down
    if (bad || !__builtin_isfinite(err)) { err = __builtin_inff(); scale = 0.f; }
    if (lane == 0) { meta_row[0] = scale; meta_row[1] = err; }
    return n;
}

// Rows [first_row, first_row + n_rows) of the store at `src` into the buffers at `codes` and `meta` (all three: the base, row 0).
// A workgroup takes whole 16-row tiles of mirror8_layout.h, its four waves rows 4 j + w of the tile in step j = 0 .. 3, and every
// lane stores its dword where mirror8_offset puts it: a row's 16-byte units are 256 bytes apart, the four waves fill 64 contiguous
// bytes at a time and the four steps the 256, all from one CU within a few microseconds, so the lines are whole when the L2 lets
// them go. No LDS, no barrier, the parent's registers: the conversion is bound by the latency of a row's two passes and lives on
// eight waves per SIMD (staging tiles in LDS for whole-line stores cost 20-30 VGPRs and took 10.3-10.5 ms for 10M rows against
// 7.9: profiles/r26). An appended range may begin or end inside a tile: a row outside it is skipped. The grid is one workgroup per
// touched tile (at most 4096), so a small append runs on a quarter of the workgroups that one per four rows would give it, each
// doing its four steps one after the other: a few microseconds at the sizes an append has.
__global__ __launch_bounds__(256) void mirror8_kernel(const float* __restrict__ src, uint32_t first_row, uint32_t n_rows, uint32_t dims,
                                                      int normalize, unsigned char* __restrict__ codes, float* __restrict__ meta,
                                                      unsigned int* __restrict__ max_norm_bits) {
    __shared__ unsigned int block_max;
    const int lane = lane_id();
    const uint32_t wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) block_max = 0u;
    __syncthreads();
    float wave_max = 0.f;
    const uint32_t end_row = first_row + n_rows;                     // (the launcher keeps a tile's last row inside 32 bits)
    const uint32_t tile0 = first_row / MIRROR8_TILE_ROWS, tile_end = (end_row + MIRROR8_TILE_ROWS - 1) / MIRROR8_TILE_ROWS;
    for (uint32_t x = 0;; ++x) {                                     // step x & 3 of the workgroup's tile number x >> 2
        const uint32_t tile = tile0 + (x >> 2) * gridDim.x + blockIdx.x;
        if (tile >= tile_end) break;
        const uint32_t r = tile * MIRROR8_TILE_ROWS + (x & 3u) * 4u + wave;
        if (r < first_row || r >= end_row) continue;
        const float n = mirror8_code_row(src + (size_t)r * dims, dims, normalize, lane, codes, r, meta + 2 * (size_t)r);
        if (n == n && n > wave_max) wave_max = n;
    }
    if (lane == 0) atomicMax(&block_max, __float_as_uint(wave_max));
    __syncthreads();
    if (threadIdx.x == 0 && block_max != 0u) atomicMax(max_norm_bits, block_max);
}

hipError_t launch_mirror8_scan(const MirrorScanArgs& args, const unsigned char* codes, const float* meta, const float* query, int metric,
                               int grid_cap, hipStream_t st) {
    if (!mirror_launch_ok(args, metric, MIRROR8_MAX_K) || codes == nullptr || meta == nullptr || args.max_bits == nullptr)
        return hipErrorInvalidValue;
    return with_code8_pass(args.n_rows, args.dims, metric, grid_cap, [&](auto s, auto m, int grid) {
        constexpr int D = decltype(s)::DIMS, M = decltype(m)::value;
        Mirror8ScanArgsQ<D> aq;
        aq.a = args;
        aq.a.lists = grid;
        aq.codes = codes;
        aq.meta = meta;
        std::memcpy(aq.q, query, sizeof(aq.q));
        launch_kernel((mirror8_scan_kernel<D, M>), dim3(grid), dim3(SCAN_THREADS), 0, st, aq);
        return launch_finish((mirror8_finish_kernel<D, M>), 1, st, aq);
    });
}

hipError_t launch_mirror8_keys(const MirrorScanArgs& args, const unsigned char* codes, const float* meta, const float* query, int metric,
                               int grid_cap, float* keys_out, hipStream_t st) {
    if (!mirror_launch_ok(args, metric, MIRROR8_MAX_K) || codes == nullptr || meta == nullptr || keys_out == nullptr) return hipErrorInvalidValue;
    return with_code8_pass(args.n_rows, args.dims, metric, grid_cap, [&](auto s, auto m, int grid) {
        constexpr int D = decltype(s)::DIMS, M = decltype(m)::value;
        Mirror8ScanArgsQ<D> aq;
        aq.a = args;
        aq.a.lists = grid;
        aq.codes = codes;
        aq.meta = meta;
        std::memcpy(aq.q, query, sizeof(aq.q));
        hipLaunchKernelGGL((mirror8_keys_kernel<D, M>), dim3(grid), dim3(SCAN_THREADS), 0, st, aq, keys_out);
        return hipGetLastError();
    });
}

hipError_t launch_mirror8_group(const MirrorGroupArgs& args, const unsigned char* codes, const float* meta, int nq, int metric,
                                int grid_cap, hipStream_t st) {
    if (!mirror_launch_ok(args.a, metric, MIRROR8_MAX_K, args.m, nq) || codes == nullptr || meta == nullptr || args.a.max_bits == nullptr)
        return hipErrorInvalidValue;
    return with_code8_pass(args.a.n_rows, args.a.dims, metric, grid_cap, [&](auto s, auto m, int grid) {
        constexpr int D = decltype(s)::DIMS, M = decltype(m)::value;
        Mirror8GroupArgs ga;
        ga.g = args;
        ga.g.a.lists = grid;
        ga.codes = codes;
        ga.meta = meta;
        return with_group_size(nq, [&](auto c) {
            launch_kernel((mirror8_scan_group_kernel<D, M, decltype(c)::value>), dim3(grid), dim3(SCAN_THREADS), 0, st, ga);
            return launch_finish((mirror8_finish_group_kernel<D, M>), nq, st, ga);
        });
    });
}

hipError_t launch_mirror8_group_masked(const MirrorGroupArgs& args, const unsigned char* codes, const float* meta, int nq, int metric,
                                       int grid_cap, hipStream_t st) {
    if (!mirror_scan_supported(args.a.dims, metric) || args.a.n_rows == 0 || nq < 1 || nq > MIRROR_MAX_NQ || codes == nullptr || meta == nullptr ||
        args.a.max_bits == nullptr)
        return hipErrorInvalidValue;
    for (int i = 0; i < nq; ++i)
        if (args.m[i].k < 1 || args.m[i].k > MIRROR8_MAX_K || args.m[i].kpad < args.m[i].k || args.m[i].query == nullptr) return hipErrorInvalidValue;
    return with_code8_pass(args.a.n_rows, args.a.dims, metric, grid_cap, [&](auto s, auto m, int grid) {
        constexpr int D = decltype(s)::DIMS, M = decltype(m)::value;
        Mirror8GroupArgs ga;
        ga.g = args;
        ga.g.a.lists = grid;
        ga.codes = codes;
        ga.meta = meta;
        switch (nq) {
            case 1: launch_kernel((mirror8_scan_masked_group_kernel<D, M, 1>), dim3(grid), dim3(SCAN_THREADS), 0, st, ga); break;
            case 2: launch_kernel((mirror8_scan_masked_group_kernel<D, M, 2>), dim3(grid), dim3(SCAN_THREADS), 0, st, ga); break;
            case 3: launch_kernel((mirror8_scan_masked_group_kernel<D, M, 3>), dim3(grid), dim3(SCAN_THREADS), 0, st, ga); break;
            default: launch_kernel((mirror8_scan_masked_group_kernel<D, M, 4>), dim3(grid), dim3(SCAN_THREADS), 0, st, ga); break;
        }
        return launch_finish((mirror8_finish_group_kernel<D, M>), nq, st, ga);
    });
}

hipError_t launch_mirror_lists_probe(const int64_t* d_keys, int nq, uint32_t n_slots, int grid, int64_t* d_partials, hipStream_t st) {
    if (d_keys == nullptr || d_partials == nullptr || nq < 1 || nq > MIRROR_MAX_NQ || n_slots == 0 || grid < 1 || grid > SCAN_KWAY_MERGE_GRID)
        return hipErrorInvalidValue;
    switch (nq) {
        case 1: hipLaunchKernelGGL(mirror_lists_probe_kernel<1>, dim3(grid), dim3(SCAN_THREADS), 0, st, d_keys, n_slots, d_partials); break;
        case 2: hipLaunchKernelGGL(mirror_lists_probe_kernel<2>, dim3(grid), dim3(SCAN_THREADS), 0, st, d_keys, n_slots, d_partials); break;
        case 3: hipLaunchKernelGGL(mirror_lists_probe_kernel<3>, dim3(grid), dim3(SCAN_THREADS), 0, st, d_keys, n_slots, d_partials); break;
        default: hipLaunchKernelGGL(mirror_lists_probe_kernel<4>, dim3(grid), dim3(SCAN_THREADS), 0, st, d_keys, n_slots, d_partials); break;
    }
    return hipGetLastError();
}

hipError_t launch_mirror8_build(const float* src, uint64_t first_row, uint32_t n_rows, uint32_t dims, int normalize, unsigned char* codes,
                                float* meta, unsigned int* max_bits, hipStream_t st) {
    if (n_rows == 0) return hipSuccess;
    if (!in_dim_list(MirrorDims{}, dims) || first_row + n_rows > 0xffffffffull - MIRROR8_TILE_ROWS) return hipErrorInvalidValue;
    uint64_t blocks = (first_row + n_rows + MIRROR8_TILE_ROWS - 1) / MIRROR8_TILE_ROWS - first_row / MIRROR8_TILE_ROWS;   // the tiles the range touches
    if (blocks > 4096) blocks = 4096;
    const int group = normalize ? scan_group_lanes(dims) : 0;
    hipLaunchKernelGGL(mirror8_kernel, dim3((unsigned)blocks), dim3(256), 0, st, src, (uint32_t)first_row, n_rows, dims, group, codes, meta, max_bits);
    return hipGetLastError();
}

}  // namespace wax
