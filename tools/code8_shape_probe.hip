// Microbenchmark behind DESIGN.md 4.1's choice of the code mirror's storage order: the scan body of the 8-bit pass (code8_pass,
// included as it is, selection and workgroup merge with it) over the SAME 10M x 384 random codes stored once row-major and once in
// mirror8_layout.h's tile order. It fills the cell MI355X_MICROARCH-style tables leave open — what a global_load_dwordx4 costs when
// it touches sixteen 64-byte half-lines 384 bytes apart instead of 1024 contiguous bytes — for the kernel that matters here.
//   variants   layout {row-major, tiled} x code loads {plain, non-temporal} x tiles per wave iteration {1, 2}
//              x the first iteration's loads {behind, ahead of} the query prologue
//   frames     on the shipped loads, the selection frame (mirror_pass.h: PassLists) as it was (plain: the general prune every time)
//              against the shipped one (sorted); and, built only here, both with a clock in them (WaveClock): per wave the time in
//              the query prologue, in in-loop prunes (with their number) and from the loop's end to the last store, reported as
//              medians over the waves of the last round
//   forms      the lone query (mirror8_scan_kernel's arguments and body) and four queries (mirror8_scan_group_kernel<.., 4>'s)
//   timing     HIP events around every launch, REPS rounds, every round runs every variant once (alternated, so drift hits all alike)
//   check      the XOR of every key of the first query's partials: equal for the variants with the same tiles per iteration (the grid,
//              hence the partials, depends on it) — a variant that read other bytes than the row-major pass, or a frame that kept
//              other keys than the plain one, shows here
// Build:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -I wax_amd/csrc tools/code8_shape_probe.hip -o code8_shape_probe
// Run:    ./code8_shape_probe [rows = 10000000] [reps = 30]      Output: one JSON line per variant and form.
#include "../wax_amd/csrc/mirror8_scan.hip"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace wax;

// mirror_scan.hip's, which the launchers of the included file refer to; the probe launches its own kernels and never calls them
bool wax::mirror_scan_supported(uint32_t dims, int) { return in_dim_list(MirrorDims{}, dims); }

namespace {

constexpr int D = 384;

#define CHECK(x)                                                                                              \
    do {                                                                                                      \
        const hipError_t e_ = (x);                                                                            \
        if (e_ != hipSuccess) {                                                                               \
            std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));          \
            std::exit(1);                                                                                     \
        }                                                                                                     \
    } while (0)

__device__ __host__ inline uint32_t mix(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return (uint32_t)x;
}

// the same code for (row, element) in both buffers; {scale, err} of a unit row coded to 8 bits
__global__ void fill_kernel(unsigned char* row_major, unsigned char* tiled, float* meta, uint32_t n) {
    const uint64_t words = (uint64_t)n * (D / 4);
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = w / (D / 4);
        const uint32_t e = (uint32_t)(w % (D / 4)) * 4;
        uint32_t v = mix(w);
        // bytes in [1, 255]: codes in [-127, 127]
        uint32_t word = 0;
        for (int i = 0; i < 4; ++i) word |= (1u + ((v >> (8 * i)) & 0xffu) % 255u) << (8 * i);
        *reinterpret_cast<uint32_t*>(row_major + r * D + e) = word;
        *reinterpret_cast<uint32_t*>(tiled + mirror8_offset(r, e, D)) = word;
        if (e == 0) { meta[2 * r] = 1.0f / (127.0f * 11.3f); meta[2 * r + 1] = 2.0e-3f + 1.0e-4f * (float)(mix(r) & 7u); }
    }
}

// Per wave: {prologue, in-loop prunes, loop's end to the last store} in ticks of wall_clock64() (10 ns), and the number of in-loop
// prunes (calls of room() that pruned), written by lane 0 with ordinary stores behind the wave's last store of partials.
constexpr int CLOCK_WORDS = 4;
__device__ unsigned long long* g_clock_out;

struct WaveClock {
    unsigned long long t0, t_loop, t_in, t_end, prune_ticks, prunes;
    __device__ __forceinline__ void begin() { t0 = wall_clock64(); prune_ticks = 0; prunes = 0; t_loop = t0; t_end = t0; }
    __device__ __forceinline__ void loop_begin() { t_loop = wall_clock64(); }
    __device__ __forceinline__ void prune_in() { t_in = wall_clock64(); }
    __device__ __forceinline__ void prune_out() { prune_ticks += wall_clock64() - t_in; ++prunes; }
    __device__ __forceinline__ void loop_end() { t_end = wall_clock64(); }
    __device__ __forceinline__ void done() {
        __builtin_amdgcn_s_waitcnt(0);                  // (the stores of the partials have left the wave)
        const unsigned long long t = wall_clock64();
        if (lane_id() == 0) {
            unsigned long long* o = g_clock_out + (size_t)(blockIdx.x * SCAN_WAVES + (threadIdx.x >> 6)) * CLOCK_WORDS;
            o[0] = t_loop - t0; o[1] = prune_ticks; o[2] = t - t_end; o[3] = prunes;
        }
    }
};

template <class LOADS, class FRAME>
__global__ __launch_bounds__(SCAN_THREADS, 2) void lone_kernel(Mirror8ScanArgsQ<D> aq) {
    __shared__ int64_t lds[MIRROR_PASS_LDS];
    code8_pass<D, M_COS, 1, false, false, LoneQuery<Mirror8ScanArgsQ<D>>, LOADS, FRAME>(aq.codes, reinterpret_cast<const f32x2*>(aq.meta), aq.a,
                                                                                      LoneQuery<Mirror8ScanArgsQ<D>>{aq.a}, nullptr, lds);
}

template <class LOADS, class FRAME>
__global__ __launch_bounds__(SCAN_THREADS, 2) void four_kernel(Mirror8GroupArgs ga) {
    __shared__ int64_t lds[4 * MIRROR_PASS_LDS];
    code8_pass<D, M_COS, 4, false, false, MemberQueries, LOADS, FRAME>(ga.codes, reinterpret_cast<const f32x2*>(ga.meta), ga.g.a,
                                                                       MemberQueries{ga.g.m}, nullptr, lds);
}

struct Variant {
    const char* layout;
    const char* loads;
    int tiles;
    bool ahead;
    bool tiled;
    const char* frame;
    bool clocked;
    void (*lone)(Mirror8ScanArgsQ<D>);
    void (*four)(Mirror8GroupArgs);
    std::vector<float> ms_lone, ms_four;
    unsigned long long xor_lone = 0, xor_four = 0;
    double clock_lone[CLOCK_WORDS] = {}, clock_four[CLOCK_WORDS] = {};      // medians over the waves, the last round's launches
};

template <bool TILED, bool NT, int TILES, bool AHEAD, class FRAME = FrameShipped>
Variant variant(const char* frame = "shipped", bool clocked = false) {
    using L = Code8Loads<TILED, NT, TILES, AHEAD>;
    Variant v{};
    v.frame = frame;
    v.clocked = clocked;
    v.layout = TILED ? "tiled" : "row-major";
    v.loads = NT ? "non-temporal" : "plain";
    v.tiles = TILES;
    v.ahead = AHEAD;
    v.tiled = TILED;
    v.lone = lone_kernel<L, FRAME>;
    v.four = four_kernel<L, FRAME>;
    return v;
}

// a selection frame on the shipped loads
template <bool SORTED, class CLOCK = NoClock>
Variant frame_variant(const char* name, bool clocked = false) {
    return variant<Code8Shipped::TILED, Code8Shipped::NT, Code8Shipped::TILES, Code8Shipped::AHEAD, PassFrame<SORTED, CLOCK>>(name, clocked);
}

double median(std::vector<float> v) {
    std::sort(v.begin(), v.end());
    return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}

unsigned long long xor_keys(const int64_t* d, size_t n) {
    std::vector<int64_t> h(n);
    CHECK(hipMemcpy(h.data(), d, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    unsigned long long x = 0;
    for (int64_t k : h) x ^= (unsigned long long)k;
    return x;
}

// medians over the waves of what the clocked launch before this call wrote
void wave_clock_medians(const unsigned long long* d_clock, int waves, double* out) {
    std::vector<unsigned long long> h((size_t)waves * CLOCK_WORDS);
    CHECK(hipMemcpy(h.data(), d_clock, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
    for (int c = 0; c < CLOCK_WORDS; ++c) {
        std::vector<unsigned long long> col(waves);
        for (int w = 0; w < waves; ++w) col[w] = h[(size_t)w * CLOCK_WORDS + c];
        std::sort(col.begin(), col.end());
        out[c] = waves % 2 ? (double)col[waves / 2] : 0.5 * ((double)col[waves / 2 - 1] + (double)col[waves / 2]);
    }
}

}  // namespace

int main(int argc, char** argv) {
    const uint32_t n = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 10000000u;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 30;
    if (n == 0 || reps < 1) return 2;

    unsigned char *d_rows = nullptr, *d_tiles = nullptr;
    float *d_meta = nullptr, *d_q = nullptr;
    int64_t* d_partials = nullptr;
    unsigned int* d_max = nullptr;
    CHECK(hipMalloc(&d_rows, mirror8_bytes(n, D)));
    CHECK(hipMalloc(&d_tiles, mirror8_bytes(n, D)));
    CHECK(hipMalloc(&d_meta, (size_t)n * 2 * sizeof(float)));
    CHECK(hipMalloc(&d_q, 4 * D * sizeof(float)));
    CHECK(hipMalloc(&d_partials, (size_t)4 * SCAN_KWAY_MERGE_GRID * MIRROR_KP * sizeof(int64_t)));
    CHECK(hipMalloc(&d_max, sizeof(unsigned int)));
    unsigned long long* d_clock = nullptr;
    const size_t clock_bytes = (size_t)SCAN_KWAY_MERGE_GRID * SCAN_WAVES * CLOCK_WORDS * sizeof(unsigned long long);
    CHECK(hipMalloc(&d_clock, clock_bytes));
    CHECK(hipMemset(d_clock, 0, clock_bytes));
    CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_clock_out), &d_clock, sizeof(d_clock)));
    CHECK(hipMemset(d_tiles, 0, mirror8_bytes(n, D)));
    hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, nullptr, d_rows, d_tiles, d_meta, n);
    CHECK(hipGetLastError());

    std::vector<float> q(4 * D);
    float qn[4];
    for (int i = 0; i < 4; ++i) {
        double s = 0;
        for (int j = 0; j < D; ++j) {
            q[i * D + j] = (float)(int)(mix(1000003ull * i + j) % 2001u) / 1000.0f - 1.0f;
            s += (double)q[i * D + j] * q[i * D + j];
        }
        qn[i] = (float)std::sqrt(s);
    }
    CHECK(hipMemcpy(d_q, q.data(), q.size() * sizeof(float), hipMemcpyHostToDevice));
    const float one = 1.0f;
    CHECK(hipMemcpy(d_max, &one, sizeof(one), hipMemcpyHostToDevice));
    CHECK(hipDeviceSynchronize());

    std::vector<Variant> vs = {
        variant<false, false, 1, false>(), variant<false, true, 1, false>(), variant<false, false, 2, false>(), variant<false, true, 2, false>(),
        variant<true, false, 1, false>(),  variant<true, true, 1, false>(),  variant<true, false, 2, false>(),  variant<true, true, 2, false>(),
        variant<false, false, 1, true>(),  variant<true, false, 1, true>(),  variant<true, true, 1, true>(),   variant<true, true, 2, true>(),
        frame_variant<false>("plain"),                   frame_variant<true>("sorted"),
        frame_variant<false, WaveClock>("plain", true),  frame_variant<true, WaveClock>("sorted", true),
    };

    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (int rep = -2; rep < reps; ++rep) {          // two rounds of warm-up
        for (Variant& v : vs) {
            const int grid = mirror_pass_grid(n, 16 * v.tiles, 0);
            MirrorScanArgs a{};
            a.partials = d_partials;
            a.max_bits = d_max;
            a.n_rows = n;
            a.dims = D;
            a.k = 10;
            a.kpad = 10;
            a.q_norm = qn[0];
            a.lists = grid;
            const unsigned char* codes = v.tiled ? d_tiles : d_rows;
            for (int form = 0; form < 2; ++form) {
                float ms = 0.f;
                if (form == 0) {
                    Mirror8ScanArgsQ<D> aq;
                    aq.a = a;
                    aq.codes = codes;
                    aq.meta = d_meta;
                    std::memcpy(aq.q, q.data(), sizeof(aq.q));
                    CHECK(hipEventRecord(e0, nullptr));
                    hipLaunchKernelGGL(v.lone, dim3(grid), dim3(SCAN_THREADS), 0, nullptr, aq);
                    CHECK(hipEventRecord(e1, nullptr));
                } else {
                    Mirror8GroupArgs ga{};
                    ga.g.a = a;
                    for (int i = 0; i < 4; ++i) {
                        ga.g.m[i].query = d_q + i * D;
                        ga.g.m[i].partials = d_partials + (size_t)i * SCAN_KWAY_MERGE_GRID * MIRROR_KP;
                        ga.g.m[i].q_norm = qn[i];
                        ga.g.m[i].k = 10;
                        ga.g.m[i].kpad = 10;
                    }
                    ga.codes = codes;
                    ga.meta = d_meta;
                    CHECK(hipEventRecord(e0, nullptr));
                    hipLaunchKernelGGL(v.four, dim3(grid), dim3(SCAN_THREADS), 0, nullptr, ga);
                    CHECK(hipEventRecord(e1, nullptr));
                }
                CHECK(hipGetLastError());
                CHECK(hipEventSynchronize(e1));
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (rep >= 0) (form == 0 ? v.ms_lone : v.ms_four).push_back(ms);
                if (rep == 0) (form == 0 ? v.xor_lone : v.xor_four) = xor_keys(d_partials, (size_t)grid * MIRROR_KP);
                if (v.clocked && rep == reps - 1) wave_clock_medians(d_clock, grid * SCAN_WAVES, form == 0 ? v.clock_lone : v.clock_four);
            }
        }
    }

    const double bytes = (double)n * D + (double)n * 8;
    for (const Variant& v : vs) {
        for (int form = 0; form < 2; ++form) {
            const std::vector<float>& ms = form == 0 ? v.ms_lone : v.ms_four;
            const double med = median(ms);
            std::printf("{\"probe\": \"code8_shape\", \"rows\": %u, \"dims\": %d, \"queries\": %d, \"layout\": \"%s\", \"loads\": \"%s\", "
                        "\"tiles_per_iteration\": %d, \"first_loads_ahead\": %s, \"frame\": \"%s\", \"clocked\": %s, \"reps\": %d, "
                        "\"ms_median\": %.4f, \"ms_min\": %.4f, \"ms_max\": %.4f, \"tb_per_s\": %.3f, \"keys_xor\": \"%016llx\"",
                        n, D, form == 0 ? 1 : 4, v.layout, v.loads, v.tiles, v.ahead ? "true" : "false", v.frame, v.clocked ? "true" : "false",
                        (int)ms.size(), med, *std::min_element(ms.begin(), ms.end()), *std::max_element(ms.begin(), ms.end()),
                        bytes / (med * 1e-3) / 1e12, form == 0 ? v.xor_lone : v.xor_four);
            if (v.clocked) {
                const double* c = form == 0 ? v.clock_lone : v.clock_four;
                std::printf(", \"wave_median_us\": {\"prologue\": %.2f, \"loop_prunes\": %.2f, \"tail\": %.2f}, \"wave_median_loop_prunes\": %.1f",
                            c[0] / 100.0, c[1] / 100.0, c[2] / 100.0, c[3]);
            }
            std::printf("}\n");
        }
    }
    return 0;
}
