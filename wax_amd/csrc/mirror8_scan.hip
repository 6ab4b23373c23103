// mirror8_scan.hip — one query (or up to four) against the 8-bit code mirror of the store, answered in f32 ("Eight bits
// per element").
//
// mirror_scan.hip's pass runs at the HBM read rate, so the next factor is again bytes per pass: one byte per element plus 8 bytes per
// row instead of two bytes per element. The structure is mirror_scan.hip's — persistent grid, GROUP lanes per row, non-temporal loads,
// the f32 query slice in VGPRs, four f32x2 chains per query, group_sum, WaveTopK<128>, block_rank_merge, MIRROR_KP keys per workgroup
// and query, and mirror_finish_body.inc for the exact re-score — with three differences:
//   the row       D bytes: code_i + 128, code_i = rint(x^_i / scale) in [-127, 127], scale = max|x^| / 127 of THAT row (x^: the f32 row,
//                 normalised for cosine as mirror_kernel does). A lane still owns 24 elements of a row: three dwordx2 loads, GROUP =
//                 D / 24 lanes, so 16 lanes cover a whole 128-byte line. v_cvt_f32_ubyteN turns a byte into a float in one full-rate
//                 instruction; the bias leaves through the first accumulator chain, which starts at -128 * (the lane's sum of q).
//   the key       meta[row] = {scale, err}, err >= ||scale * code - x^||_2 (measured per row by mirror8_kernel, rounded up). With
//                 s = scale * sum_i q_i code_i:  |s - q.x^| <= ||q|| err, so
//                     cosine  lb = 1 - s / ||q|| - err          dot  lb = 1 - s - ||q|| err
//                 is a LOWER BOUND of the row's distance (up to the slack below). A NaN lb, and err = +inf, give -inf: such a row is
//                 always a candidate and is re-scored exactly.
//   certificate   lb_KP - slack > d_k, strict. Every row outside the candidates has lb >= lb_KP, hence an exact distance
//                 >= lb_KP - slack > d_k. slack (mirror8_slack) holds what err does not — see there.
#include <cstddef>
#include <cstring>

#include "kernels.h"
#include "row_math.h"
#include "topk.h"

namespace wax {

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int MIRROR8_UNROLL = 8;     // row groups in flight per wave: 3 x 8 dwordx2 loads per lane = the bytes in flight of the bf16 kernel

using Mirror8Dims = DimList<384, 768>;

// lanes per row: three dwordx2 (24 codes) per lane and row
template <int DIMS> struct Mirror8Shape { static constexpr int D8 = DIMS / 8, GROUP = D8 / 3; };

// four biased codes in one dword -> floats (element 4i is the low byte); each conversion is one v_cvt_f32_ubyteN
__device__ inline f32x2 bytes_lo(unsigned int w) {
    f32x2 r;
    r.x = (float)(w & 0xffu);
    r.y = (float)((w >> 8) & 0xffu);
    return r;
}
__device__ inline f32x2 bytes_hi(unsigned int w) {
    f32x2 r;
    r.x = (float)((w >> 16) & 0xffu);
    r.y = (float)(w >> 24);
    return r;
}

// the wave's maximum in every lane (the build kernel only)
__device__ inline float wave_max64(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// -128 * (the sum of a lane's 24 query elements): where the first chain starts. 128 * x is exact; the sum's own rounding is in the slack.
template <int LOADS>
__device__ inline float bias_start(const f32x2 (&q)[LOADS][4]) {
    f32x2 t = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < LOADS; ++j) t += (q[j][0] + q[j][1]) + (q[j][2] + q[j][3]);
    return -128.0f * (t.x + t.y);
}

// One row of one query: the lane's three loads (already floats, biased) into four chains, the group's sum, the lower-bound key
// distance. The lone and the group kernel both call this, so a query's keys do not depend on what it rode with.
template <int GROUP, int LOADS, int METRIC>
__device__ inline float row_lower_bound(const f32x2 (&q)[LOADS][4], const f32x2 (&w)[LOADS][4], float start, float scale, float err,
                                        float inv_qn, float q_norm) {
    f32x2 acc[4] = {{start, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
    for (int j = 0; j < LOADS; ++j) {
        acc[0] = __builtin_elementwise_fma(q[j][0], w[j][0], acc[0]);
        acc[1] = __builtin_elementwise_fma(q[j][1], w[j][1], acc[1]);
        acc[2] = __builtin_elementwise_fma(q[j][2], w[j][2], acc[2]);
        acc[3] = __builtin_elementwise_fma(q[j][3], w[j][3], acc[3]);
    }
    const f32x2 s2 = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    const float s = scale * group_sum<GROUP>(s2.x + s2.y);
    float lb = METRIC == M_COS ? (1.0f - s * inv_qn) - err : (1.0f - s) - q_norm * err;
    lb = (lb != lb) ? -__builtin_inff() : lb;
    return lb + 0.0f;
}

// What the per-row err does not hold, as a bound on (lb as computed) - (the row's exact distance as row_distance computes it):
//  (a) the f32 accumulation of sum_i q_i (code_i + 128) - 128 Q, Q the lane's rounded sum of its q_i. Every path from a term to the
//      group's total crosses at most 11 roundings (3 fma, 2 + 1 adds of the lane's tree, <= 5 DPP adds), Q's own sum 23; the terms'
//      magnitudes sum to at most (255 + 128) ||q||_1, so with u = 2^-24
//          |computed - sum_i q_i code_i| <= (11 * 383 + 23 * 128) u ||q||_1 (1 + O(u)) < 8192 u sqrt(D) ||q||,
//      times scale <= max||v|| / 127 (cosine: 1 / 127);
//  (b) 3 D u ||q|| max||v|| for the f32 sums and normalisations on either side, as in the bf16 certificate;
//  (c) the roundings of scale * acc, / ||q||, the two subtractions, and the exact distance's own ~1e-6: 3e-6 (cosine),
//      3e-6 (1 + ||q|| max||v||) (dot) — a row that matters has |lb| <= 2 (1 + ||q|| max||v||).
// Cosine divides by ||q||, so both norms are 1 there.
template <int DIMS, int METRIC>
__device__ inline float mirror8_slack(float q_norm, const unsigned int* max_bits) {
    const double qn = METRIC == M_COS ? 1.0 + 1e-6 : (double)q_norm;
    const double vn = METRIC == M_COS ? 1.0 + 1e-6 : (double)__uint_as_float(max_bits[0]);
    const double u = 5.97e-8;
    const double acc = 8192.0 * u * __builtin_sqrt((double)DIMS) / 127.0;
    const double both = (acc + 3.0 * (double)DIMS * u) * qn * vn * 1.001;
    const float s = METRIC == M_COS ? (float)(both + 3e-6) : (float)(both + 3e-6 * (1.0 + qn * vn));
    return nextafterf(s, __builtin_inff());
}

}  // namespace

template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS) void mirror8_scan_kernel(Mirror8ScanArgsQ<DIMS> aq) {
    constexpr int D8 = Mirror8Shape<DIMS>::D8;      // dwordx2 (8 codes) per row
    constexpr int GROUP = Mirror8Shape<DIMS>::GROUP;
    constexpr int LOADS = D8 / GROUP;
    constexpr int RPW = WAVE / GROUP;
    constexpr int RPC = RPW * MIRROR8_UNROLL;
    constexpr int CAP = 128;
    static_assert(LOADS == 3 && D8 % GROUP == 0, "three dwordx2 per lane and row");
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
    const f32x4* q4 = reinterpret_cast<const f32x4*>(ka + offsetof(Mirror8ScanArgsQ<DIMS>, q));
    f32x2 q[LOADS][4];
#pragma unroll
    for (int j = 0; j < LOADS; ++j) {
        const f32x4 lo = q4[2 * (gl + j * GROUP)], hi = q4[2 * (gl + j * GROUP) + 1];
        q[j][0] = lo.xy; q[j][1] = lo.zw; q[j][2] = hi.xy; q[j][3] = hi.zw;
    }
    const float start = bias_start<LOADS>(q);
    const float inv_qn = a.q_norm > COS_NORM_FLOOR ? 1.0f / a.q_norm : 0.0f;

    const u32x2* __restrict__ codes2 = reinterpret_cast<const u32x2*>(aq.codes);
    const f32x2* __restrict__ meta2 = reinterpret_cast<const f32x2*>(aq.meta);
    WaveTopK<CAP> tk;
    tk.init(lds + wave * CAP, MIRROR_KP);

    const uint32_t nchunks = (n + RPC - 1) / RPC;
    const uint32_t gwave = blockIdx.x * SCAN_WAVES + wave;
    const uint32_t nwaves = gridDim.x * SCAN_WAVES;

    for (uint32_t chunk = gwave; chunk < nchunks; chunk += nwaves) {
        const uint32_t rbase = chunk * RPC + sub;
        tk.make_room(RPC);
        u32x2 v[MIRROR8_UNROLL][LOADS];
        f32x2 mt[MIRROR8_UNROLL];
#pragma unroll
        for (int u = 0; u < MIRROR8_UNROLL; ++u) {
            const uint32_t r = rbase + u * RPW;
            const uint32_t rc = r < n ? r : n - 1;  // clamp: tail lanes re-read the last row, result discarded
            const u32x2* p = codes2 + (size_t)rc * D8 + gl;
#pragma unroll
            for (int j = 0; j < LOADS; ++j) v[u][j] = __builtin_nontemporal_load(p + j * GROUP);
            mt[u] = __builtin_nontemporal_load(meta2 + rc);     // (every lane of the group: one address, one request)
        }
#pragma unroll
        for (int u = 0; u < MIRROR8_UNROLL; ++u) {
            f32x2 w[LOADS][4];
#pragma unroll
            for (int j = 0; j < LOADS; ++j) {
                w[j][0] = bytes_lo(v[u][j].x); w[j][1] = bytes_hi(v[u][j].x); w[j][2] = bytes_lo(v[u][j].y); w[j][3] = bytes_hi(v[u][j].y);
            }
            const float lb = row_lower_bound<GROUP, LOADS, METRIC>(q, w, start, mt[u].x, mt[u].y, inv_qn, a.q_norm);
            const uint32_t r = rbase + u * RPW;
            tk.push(make_key(lb, a.row_base + r), owner && (r < n));
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

#define MIRROR_FINISH_EPS mirror8_slack<DIMS, METRIC>(a.q_norm, a.max_bits)

template <int DIMS, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS) void mirror8_finish_kernel(Mirror8ScanArgsQ<DIMS> aq) {
    const MirrorScanArgs& a = aq.a;
#define MIRROR_FINISH_QUERY reinterpret_cast<const f32x4*>((const char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(Mirror8ScanArgsQ<DIMS>, q))
#include "mirror_finish_body.inc"
#undef MIRROR_FINISH_QUERY
}

// ---- several queries per pass: mirror_scan_group_kernel's shape — loads, clamp and conversions shared, row_lower_bound per query ----
template <int DIMS, int METRIC, int NQ>
__global__ __launch_bounds__(SCAN_THREADS) void mirror8_scan_group_kernel(Mirror8GroupArgs ga) {
    constexpr int D8 = Mirror8Shape<DIMS>::D8;
    constexpr int GROUP = Mirror8Shape<DIMS>::GROUP;
    constexpr int LOADS = D8 / GROUP;
    constexpr int RPW = WAVE / GROUP;
    constexpr int RPC = RPW * MIRROR8_UNROLL;
    constexpr int CAP = 128;
    constexpr int PER_Q = SCAN_WAVES * CAP + SCAN_WAVES + MIRROR_KP;
    static_assert(LOADS == 3 && D8 % GROUP == 0, "three dwordx2 per lane and row");
    static_assert(NQ >= 2 && NQ <= MIRROR_MAX_NQ, "queries per pass");
    const MirrorGroupArgs& g = ga.g;
    const MirrorScanArgs& a = g.a;
    __shared__ int64_t lds[NQ * PER_Q];

    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const int sub = lane / GROUP;
    const int gl = lane % GROUP;
    const bool owner = (gl == GROUP - 1);
    const uint32_t n = a.n_rows;

    f32x2 q[NQ][LOADS][4];
    float inv_qn[NQ], start[NQ], qn[NQ];
    WaveTopK<CAP> tk[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const f32x4* q4 = reinterpret_cast<const f32x4*>(g.m[i].query);
#pragma unroll
        for (int j = 0; j < LOADS; ++j) {
            const f32x4 lo = q4[2 * (gl + j * GROUP)], hi = q4[2 * (gl + j * GROUP) + 1];
            q[i][j][0] = lo.xy; q[i][j][1] = lo.zw; q[i][j][2] = hi.xy; q[i][j][3] = hi.zw;
        }
        start[i] = bias_start<LOADS>(q[i]);
        qn[i] = g.m[i].q_norm;
        inv_qn[i] = qn[i] > COS_NORM_FLOOR ? 1.0f / qn[i] : 0.0f;
        tk[i].init(lds + i * PER_Q + wave * CAP, MIRROR_KP);
    }

    const u32x2* __restrict__ codes2 = reinterpret_cast<const u32x2*>(ga.codes);
    const f32x2* __restrict__ meta2 = reinterpret_cast<const f32x2*>(ga.meta);
    const uint32_t nchunks = (n + RPC - 1) / RPC;
    const uint32_t gwave = blockIdx.x * SCAN_WAVES + wave;
    const uint32_t nwaves = gridDim.x * SCAN_WAVES;

    for (uint32_t chunk = gwave; chunk < nchunks; chunk += nwaves) {
        const uint32_t rbase = chunk * RPC + sub;
#pragma unroll
        for (int i = 0; i < NQ; ++i) tk[i].make_room(RPC);
        u32x2 v[MIRROR8_UNROLL][LOADS];
        f32x2 mt[MIRROR8_UNROLL];
#pragma unroll
        for (int u = 0; u < MIRROR8_UNROLL; ++u) {
            const uint32_t r = rbase + u * RPW;
            const uint32_t rc = r < n ? r : n - 1;  // clamp: tail lanes re-read the last row, result discarded
            const u32x2* p = codes2 + (size_t)rc * D8 + gl;
#pragma unroll
            for (int j = 0; j < LOADS; ++j) v[u][j] = __builtin_nontemporal_load(p + j * GROUP);
            mt[u] = __builtin_nontemporal_load(meta2 + rc);
        }
#pragma unroll
        for (int u = 0; u < MIRROR8_UNROLL; ++u) {
            f32x2 w[LOADS][4];              // converted once, used by every query
#pragma unroll
            for (int j = 0; j < LOADS; ++j) {
                w[j][0] = bytes_lo(v[u][j].x); w[j][1] = bytes_hi(v[u][j].x); w[j][2] = bytes_lo(v[u][j].y); w[j][3] = bytes_hi(v[u][j].y);
            }
            const uint32_t r = rbase + u * RPW;
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                const float lb = row_lower_bound<GROUP, LOADS, METRIC>(q[i], w, start[i], mt[u].x, mt[u].y, inv_qn[i], qn[i]);
                tk[i].push(make_key(lb, a.row_base + r), owner && (r < n));
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
__global__ __launch_bounds__(SCAN_THREADS) void mirror8_finish_group_kernel(Mirror8GroupArgs ga) {
    const MirrorMember& m = ga.g.m[blockIdx.x];
    MirrorScanArgs a = ga.g.a;
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

#undef MIRROR_FINISH_EPS

// ---------------------------------------------------------------------------
// f32 rows -> biased codes + {scale, err}. One wave per row. The f32 STORE is read, never the bf16 mirror (the errors would add).
//   x^      cosine: v * (1 / sqrt(m)), m = the scan's own sum of squares (scan_order_norm2), a row the scan scores 0 (sqrt(m) <= 1e-6,
//           NaN) becomes zero — mirror_kernel's rule and expression; dot: v.
//   scale   max|x^| / 127; code = rint(x^ / scale) clamped to +-127 (a zero row: scale 0, codes 0).
//   err     sqrt(sum_i fma(scale, code_i, -x^_i)^2): each difference is rounded once (relative 2^-24), the sum of D squares and the root
//           lose at most (D / 2 + 2) 2^-24 relative, so err * (1 + D 2^-23), then nextafter, is an upper bound. The differences are
//           squared and summed in units of 2^ex, scale = f * 2^ex (ldexpf: exact), and the root is scaled back: for a row of ordinary
//           magnitude that changes no bit, and a row of 1e-30 or 1e+21 — whose squared differences are 0 or +inf in f32 — gets the err
//           it has instead of 2^-149 (no bound at all) or +inf.
//   A row with an inf / NaN element (or whose scale or err is still not finite) gets err = +inf and scale 0.
__global__ __launch_bounds__(256) void mirror8_kernel(const float* __restrict__ src, uint32_t n_rows, uint32_t dims, int normalize,
                                                      unsigned char* __restrict__ codes, float* __restrict__ meta,
                                                      unsigned int* __restrict__ max_norm_bits) {
    __shared__ unsigned int block_max;
    const int lane = lane_id();
    const uint32_t gwave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t nwaves = gridDim.x * 4;
    const uint32_t d4 = dims >> 2;
    if (threadIdx.x == 0) block_max = 0u;
    __syncthreads();
    float wave_max = 0.f;
    for (uint32_t r = gwave; r < n_rows; r += nwaves) {
        const float* row = src + (size_t)r * dims;
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
        unsigned int* out = reinterpret_cast<unsigned int*>(codes + (size_t)r * dims);
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
            out[c] = word;
        }
        e2 = group_sum<64>(e2);
        e2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e2), 63));
        float errn = sqrtf(e2) * (1.0f + (float)dims * 1.1920929e-7f);
        errn = nextafterf(errn, __builtin_inff());
        float err = ldexpf(errn, ex);
        if (ldexpf(err, -ex) < errn) err = nextafterf(err, __builtin_inff());     // back in the subnormal range: rounded up, never down
        if (bad || !__builtin_isfinite(err)) { err = __builtin_inff(); scale = 0.f; }
        if (lane == 0) { meta[2 * (size_t)r] = scale; meta[2 * (size_t)r + 1] = err; }
        if (n == n && n > wave_max) wave_max = n;
    }
    if (lane == 0) atomicMax(&block_max, __float_as_uint(wave_max));
    __syncthreads();
    if (threadIdx.x == 0 && block_max != 0u) atomicMax(max_norm_bits, block_max);
}

namespace {
template <int DIMS, int METRIC>
hipError_t launch_mirror8_dims(const MirrorScanArgs& args, const unsigned char* codes, const float* meta, const float* query, int grid, hipStream_t st) {
    Mirror8ScanArgsQ<DIMS> aq;
    aq.a = args;
    aq.a.lists = grid;
    aq.codes = codes;
    aq.meta = meta;
    std::memcpy(aq.q, query, sizeof(aq.q));
    launch_kernel((mirror8_scan_kernel<DIMS, METRIC>), dim3(grid), dim3(SCAN_THREADS), 0, st, aq);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL((mirror8_finish_kernel<DIMS, METRIC>), dim3(1), dim3(SCAN_THREADS), 0, st, aq);
    return hipGetLastError();
}
template <int DIMS, int METRIC>
hipError_t launch_group8_dims(const MirrorGroupArgs& args, const unsigned char* codes, const float* meta, int nq, int grid, hipStream_t st) {
    Mirror8GroupArgs ga;
    ga.g = args;
    ga.g.a.lists = grid;
    ga.codes = codes;
    ga.meta = meta;
    switch (nq) {
        case 2: launch_kernel((mirror8_scan_group_kernel<DIMS, METRIC, 2>), dim3(grid), dim3(SCAN_THREADS), 0, st, ga); break;
        case 3: launch_kernel((mirror8_scan_group_kernel<DIMS, METRIC, 3>), dim3(grid), dim3(SCAN_THREADS), 0, st, ga); break;
        case 4: launch_kernel((mirror8_scan_group_kernel<DIMS, METRIC, 4>), dim3(grid), dim3(SCAN_THREADS), 0, st, ga); break;
        default: return hipErrorInvalidValue;
    }
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL((mirror8_finish_group_kernel<DIMS, METRIC>), dim3(nq), dim3(SCAN_THREADS), 0, st, ga);
    return hipGetLastError();
}
}  // namespace

int mirror8_grid_for(uint32_t n_rows, uint32_t dims, int grid_cap) {
    // mirror_grid_for's rule with this unit's rows per wave iteration
    if (grid_cap <= 0) grid_cap = 512;
    if (grid_cap > SCAN_KWAY_MERGE_GRID) grid_cap = SCAN_KWAY_MERGE_GRID;
    const uint64_t rpc = (uint64_t)(WAVE / (dims / 24)) * MIRROR8_UNROLL;
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

hipError_t launch_mirror8_scan(const MirrorScanArgs& args, const unsigned char* codes, const float* meta, const float* query, int metric,
                               int grid_cap, hipStream_t st) {
    if (!mirror_scan_supported(args.dims, metric) || args.k < 1 || args.k > MIRROR8_MAX_K || args.kpad < args.k || args.n_rows == 0 ||
        codes == nullptr || meta == nullptr || args.max_bits == nullptr)
        return hipErrorInvalidValue;
    const int grid = mirror8_grid_for(args.n_rows, args.dims, grid_cap);
    return with_scan_shape(Mirror8Dims{}, args.dims, [&](auto s) {
        return with_metric_in<M_COS, M_DOT>(metric, [&](auto m) {
            return launch_mirror8_dims<decltype(s)::DIMS, decltype(m)::value>(args, codes, meta, query, grid, st);
        }, hipErrorInvalidValue);
    }, hipErrorInvalidValue);
}

hipError_t launch_mirror8_group(const MirrorGroupArgs& args, const unsigned char* codes, const float* meta, int nq, int metric,
                                int grid_cap, hipStream_t st) {
    if (!mirror_scan_supported(args.a.dims, metric) || nq < 2 || nq > MIRROR_MAX_NQ || args.a.n_rows == 0 || codes == nullptr ||
        meta == nullptr || args.a.max_bits == nullptr)
        return hipErrorInvalidValue;
    for (int i = 0; i < nq; ++i)
        if (args.m[i].k < 1 || args.m[i].k > MIRROR8_MAX_K || args.m[i].kpad < args.m[i].k || args.m[i].query == nullptr) return hipErrorInvalidValue;
    const int grid = mirror8_grid_for(args.a.n_rows, args.a.dims, grid_cap);
    return with_scan_shape(Mirror8Dims{}, args.a.dims, [&](auto s) {
        return with_metric_in<M_COS, M_DOT>(metric, [&](auto m) {
            return launch_group8_dims<decltype(s)::DIMS, decltype(m)::value>(args, codes, meta, nq, grid, st);
        }, hipErrorInvalidValue);
    }, hipErrorInvalidValue);
}

hipError_t launch_mirror8_build(const float* src, uint32_t n_rows, uint32_t dims, int normalize, unsigned char* codes, float* meta,
                                unsigned int* max_bits, hipStream_t st) {
    if (n_rows == 0) return hipSuccess;
    if (!in_dim_list(Mirror8Dims{}, dims)) return hipErrorInvalidValue;
    uint64_t blocks = ((uint64_t)n_rows + 3) / 4;
    if (blocks > 4096) blocks = 4096;
    const int group = normalize ? scan_group_lanes(dims) : 0;
    hipLaunchKernelGGL(mirror8_kernel, dim3((unsigned)blocks), dim3(256), 0, st, src, n_rows, dims, group, codes, meta, max_bits);
    return hipGetLastError();
}

}  // namespace wax
