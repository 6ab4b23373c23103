// mirror8_scan.hip — one query (or up to four) against the 8-bit code mirror of the store, answered in f32 ("Eight bits
// per element").
//
// mirror_scan.hip's pass runs at the HBM read rate, so the next factor is again bytes per pass: one byte per element plus 8 bytes per
// row instead of two bytes per element. The pass is mirror_scan.hip's — mirror_pass (mirror_pass.h) for the scan of one query
// (mirror8_scan_kernel) or of 2-4 (mirror8_scan_group_kernel), mirror_finish (mirror_finish.h) for the exact re-score — over another
// row format, Code8Rows, with another certificate:
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
#include <cstring>

#include "mirror_finish.h"
#include "mirror_pass.h"

namespace wax {

namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// the wave's maximum in every lane (the build kernel only)
__device__ inline float wave_max64(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// The code mirror as a row format of mirror_pass: three dwordx2 (24 codes) per lane and row, 8 row groups in flight (3 x 8 dwordx2
// loads per lane = the bytes in flight of the bf16 pass), {scale, err} beside every row, the key a lower bound of the distance.
struct Code8Rows {
    using Vec = u32x2;
    using Side = f32x2;                   // {scale, err}
    static constexpr int UNROLL = 8;
    static __device__ __forceinline__ Side side(const Side* meta, uint32_t r) {
        return __builtin_nontemporal_load(meta + r);     // (every lane of the group: one address, one request)
    }
    // four biased codes in one dword -> floats (element 4i is the low byte); each conversion is one v_cvt_f32_ubyteN. Chains 0 and 1
    // take the low and the high pair of dword x, chains 2 and 3 those of dword y.
    static __device__ __forceinline__ f32x2 part(const Vec& v, int c) {
        const unsigned int w = v[c >> 1];
        f32x2 r;
        r.x = (c & 1) ? (float)((w >> 16) & 0xffu) : (float)(w & 0xffu);
        r.y = (c & 1) ? (float)(w >> 24) : (float)((w >> 8) & 0xffu);
        return r;
    }
    // -128 * (the sum of a lane's 24 query elements): the bias leaves through the first chain. 128 * x is exact; the sum's own rounding
    // is in the slack.
    static __device__ __forceinline__ float start(const f32x2 (&q)[3][4]) {
        f32x2 t = {0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 3; ++j) t += (q[j][0] + q[j][1]) + (q[j][2] + q[j][3]);
        return -128.0f * (t.x + t.y);
    }
    template <int METRIC>
    static __device__ __forceinline__ float key(float sum, Side meta, float inv_qn, float q_norm) {
        const float s = meta.x * sum;
        const float lb = METRIC == M_COS ? (1.0f - s * inv_qn) - meta.y : (1.0f - s) - q_norm * meta.y;
        return (lb != lb) ? -__builtin_inff() : lb;
    }
};

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
__global__ __launch_bounds__(SCAN_THREADS) void mirror8_scan_kernel(Mirror8ScanArgsQ<DIMS> aq) {
    __shared__ int64_t lds[MIRROR_PASS_LDS];
    mirror_pass<Code8Rows, DIMS, METRIC, 1, false>(reinterpret_cast<const u32x2*>(aq.codes), reinterpret_cast<const f32x2*>(aq.meta), aq.a,
                                                    LoneQuery<Mirror8ScanArgsQ<DIMS>>{aq.a}, nullptr, lds);
}

template <int DIMS, int METRIC, int NQ>
__global__ __launch_bounds__(SCAN_THREADS) void mirror8_scan_group_kernel(Mirror8GroupArgs ga) {
    static_assert(NQ >= 2, "a lone query has mirror8_scan_kernel");
    __shared__ int64_t lds[NQ * MIRROR_PASS_LDS];
    mirror_pass<Code8Rows, DIMS, METRIC, NQ, false>(reinterpret_cast<const u32x2*>(ga.codes), reinterpret_cast<const f32x2*>(ga.meta), ga.g.a,
                                                     MemberQueries{ga.g.m}, nullptr, lds);
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

hipError_t launch_mirror8_scan(const MirrorScanArgs& args, const unsigned char* codes, const float* meta, const float* query, int metric,
                               int grid_cap, hipStream_t st) {
    if (!mirror_launch_ok(args, metric, MIRROR8_MAX_K) || codes == nullptr || meta == nullptr || args.max_bits == nullptr)
        return hipErrorInvalidValue;
    return with_mirror_pass<Code8Rows>(args.n_rows, args.dims, metric, grid_cap, [&](auto s, auto m, int grid) {
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

hipError_t launch_mirror8_group(const MirrorGroupArgs& args, const unsigned char* codes, const float* meta, int nq, int metric,
                                int grid_cap, hipStream_t st) {
    if (!mirror_launch_ok(args.a, metric, MIRROR8_MAX_K, args.m, nq) || codes == nullptr || meta == nullptr || args.a.max_bits == nullptr)
        return hipErrorInvalidValue;
    return with_mirror_pass<Code8Rows>(args.a.n_rows, args.a.dims, metric, grid_cap, [&](auto s, auto m, int grid) {
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

hipError_t launch_mirror8_build(const float* src, uint32_t n_rows, uint32_t dims, int normalize, unsigned char* codes, float* meta,
                                unsigned int* max_bits, hipStream_t st) {
    if (n_rows == 0) return hipSuccess;
    if (!in_dim_list(MirrorDims{}, dims)) return hipErrorInvalidValue;
    uint64_t blocks = ((uint64_t)n_rows + 3) / 4;
    if (blocks > 4096) blocks = 4096;
    const int group = normalize ? scan_group_lanes(dims) : 0;
    hipLaunchKernelGGL(mirror8_kernel, dim3((unsigned)blocks), dim3(256), 0, st, src, n_rows, dims, group, codes, meta, max_bits);
    return hipGetLastError();
}

}  // namespace wax
