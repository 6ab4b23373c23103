// batch_ksplit.hip — the K-split register-resident filtering GEMM: the filtering launch of the one-pass batched pipeline for cosine
// and dot stores at 1 024 and 1 536 dimensions ("The K-split filtering GEMM"; wax_hip_search_batch_dims, api_batch_dims.inc).
//
// batch_gemm_rq_kernel (batch.hip) keeps a wave's 32 queries x D resident as MFMA A fragments: D / 4 VGPRs, 256 / 384 at these
// dimensions, which do not fit at two waves per SIMD. Here TWO waves share 32 queries and each keeps HALF of K.
//
//   batch_gemm_ks_kernel<D>   512 threads, 8 waves, two per SIMD. Waves w and w + 4 own queries [32 w, 32 w + 32) of the workgroup's
//                             128; wave half h = wave >> 2 keeps k-steps [h KS/2, (h + 1) KS/2) of them as v_mfma_f32_32x32x16_bf16
//                             fragments (128 VGPRs at 1 024-d, 192 at 1 536-d), read from the prep kernel's fragment-ordered copy
//                             (GemmArgs::qf). nq_pad / 128 query groups of 256 / groups persistent workgroups; workgroup bidx of a
//                             group walks the 32-row tiles bidx, bidx + per_group, ...
//   data movement             a tile streams as K-pieces: step s of a tile brings, for each half, 32 rows x 256 columns of that half's
//                             K range — two images of 32 x (512 + 16) bytes, 33 KB a pair, exactly 33 LDS-DMA requests of 1 KB
//                             (global_load_lds_dwordx4; wave 0 issues five, the others four). The row stride of 528 bytes keeps
//                             ds_read_b128 conflict-free ((528 / 4) % 64 == 4). A ring of three pairs (99 KB): while step g is
//                             multiplied, step g + 1 has landed and step g + 2 is in flight — across the step's barrier. A tile is
//                             two steps at 1 024-d and three at 1 536-d, 16 MFMAs per wave and step. Requests are not clamped: a pad
//                             slot fetches the 16 bytes behind its piece, the last tile rows behind the store — all inside the mirror's
//                             BATCH_MIRROR_SLACK_ROWS and never used (rows >= slab_end are masked by the selection).
//   combining the halves      each wave accumulates one f32x16 over its K half. Behind its last step of a tile the upper wave writes
//                             its 16 partials per lane to a 16-KB area [pair][register quad][lane] (four ds_write_b128, consecutive
//                             lanes 16 bytes apart); behind the step's barrier the lower wave reads them, adds and selects while the
//                             upper wave goes on to the next tile. One area is enough: the lower wave has consumed it before it
//                             arrives at the NEXT barrier, and the upper wave writes it again only behind that barrier (a tile is at
//                             least two steps).
//   selection                 batch_gemm_kernel's contract: d = (1 - acc) + 0.0f <= tau[q] for rows < slab_end (a NaN fails), key
//                             make_key(d, row_base + row), appended at atomicAdd(&cand_count[q * CAND_COUNT_STRIDE], 1) and stored
//                             only below cand_cap; the count is never clamped. The hot test is batch_gemm_rq_kernel's: a subtraction
//                             and a funnel shift per accumulator against a conservative bound, one ballot per tile. The cold path
//                             walks the lane's sixteen bits; its returning atomic drains the lane's request queue, which only a tile
//                             with survivors pays.
//   no LDS access the compiler can see sits inside the tile loop (batch.hip explains why: hipcc would drain the request queue in front
//   of it); fragments, partials and bounds move by inline ds_read_b128 / ds_write_b128 with counted lgkmcnt.
//
// Exactness. The certificate is unchanged: eps carries 3 D 2^-24 of the product of the norms for the f32 accumulation of D exact
// bf16 x bf16 products, whatever the order — a sum of D terms along any tree rounds at most D - 1 times on a path from a product to the
// result, each rounding at most 2^-24 of a partial sum that the product of the norms bounds. Here a path is at most D / 2 - 1
// roundings inside a half (the MFMA's own tree is no deeper than a sequential chain) plus ONE for partial_lo + partial_hi: D / 2
// against the D - 1 of a single chain, and under D 2^-24 with the term's factor 3 untouched.
//
// Deviations from the planned form: the lane's sixteen bounds are re-read from LDS per tile at both dimensions (one code path; at
// 1 536-d they do not fit beside 192 registers of fragments), and the cold path is a walk over the lane's bits with one global
// returning add per survivor, not a staged append. Every list, count and key is written with vector stores.
#include <type_traits>

#include "kernels.h"
#include "row_math.h"

namespace wax {

typedef float ks_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 ks_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int ks_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void ks_lds_void;
typedef __attribute__((address_space(1))) const void ks_global_cvoid;

// f(std::integral_constant<int, I>{}) for I in [I0, N): inline-asm immediates and register indices need constant expressions
template <int I, int N, typename F>
__device__ __forceinline__ void ks_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        ks_static_for<I + 1, N>(f);
    }
}

constexpr int KS_QUERIES = 128;                      // queries per workgroup: four wave pairs of 32
constexpr int KS_TROWS = 32;                         // rows per tile
constexpr int KS_STEP_COLS = 256;                    // columns of each K half per step
constexpr int KS_ROW_B = KS_STEP_COLS * 2 + 16;      // LDS row stride of a piece
constexpr int KS_PIECE_B = KS_TROWS * KS_ROW_B;      // one half's image of a step
constexpr int KS_PAIR_B = 2 * KS_PIECE_B;            // lower + upper
constexpr int KS_NRING = 3;
constexpr int KS_REQS = KS_PAIR_B / 1024;            // 1-KB LDS-DMA requests per step (33)
constexpr int KS_PPW = (KS_REQS + 7) / 8;            // requests per wave: waves below KS_FULL_WAVES issue PPW, the others PPW - 1
constexpr int KS_FULL_WAVES = KS_REQS % 8 == 0 ? 8 : KS_REQS % 8;
constexpr int KS_SLOTS_PER_ROW = KS_ROW_B / 16;      // 16-byte slots per padded row (33)
constexpr int KS_PART_B = 4 * 4 * 64 * 16;           // [pair][register quad][lane] x 16 bytes
constexpr int KS_SIM_B = 4 * 32 * 4;                 // [pair][query] conservative similarity bounds
constexpr size_t KS_SMEM = (size_t)KS_NRING * KS_PAIR_B + KS_PART_B + KS_SIM_B;
static_assert(KS_PAIR_B % 1024 == 0, "a step is a whole number of 1-KB requests");
static_assert((KS_ROW_B / 4) % 64 == 4, "row stride must keep ds_read_b128 conflict-free");
static_assert(KS_TROWS + 2 <= (int)BATCH_MIRROR_SLACK_ROWS, "the un-clamped requests of the last tile stay inside the mirror's slack rows");
static_assert(KS_SMEM <= 160 * 1024, "LDS budget of one CU");

template <int N>
__device__ inline void ks_wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

template <int D>
__global__ __launch_bounds__(512, 2) void batch_gemm_ks_kernel(GemmArgs a, uint32_t blocks_per_group) {
    constexpr int KS = D / 16;                       // MFMA k-steps of a row
    constexpr int KH = KS / 2;                       // ... of one K half = resident fragments per wave
    constexpr int FPS = KS_STEP_COLS / 16;           // fragments (= MFMAs) per wave and step
    constexpr int SPT = KH / FPS;                    // steps per tile
    constexpr int AHEAD = 3, RING = AHEAD + 1;       // B-fragment read-ahead
    static_assert(D % 512 == 0 && SPT >= 2, "whole steps; the partial area is rewritten two barriers after it is read");
    extern __shared__ __attribute__((aligned(16))) unsigned char ks_smem[];
    float* sim_s = reinterpret_cast<float*>(ks_smem + KS_NRING * KS_PAIR_B + KS_PART_B);

    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = wave >> 2, pair = wave & 3;     // wave-uniform
    const uint32_t group = blockIdx.x / blocks_per_group;
    const uint32_t bidx = blockIdx.x % blocks_per_group;
    const uint32_t q0 = group * (uint32_t)KS_QUERIES + (uint32_t)pair * 32u;   // the pair's 32 queries

    // A fragments of this wave's K half: lane l holds query (l & 31), k = 16 ks + 8 (l >> 5) .. + 7
    ks_bf16x8 fa[KH];
    {
        if (a.qf != nullptr) {   // fragment order: one contiguous 1-KB run per 32 queries and k-step
            const ks_u32x4* qp = reinterpret_cast<const ks_u32x4*>(a.qf) + ((size_t)(q0 >> 5) * KS + (size_t)(half * KH)) * 64 + lane;
#pragma unroll
            for (int i = 0; i < KH; ++i) fa[i] = __builtin_bit_cast(ks_bf16x8, qp[i * 64]);
        } else {
            const ks_u32x4* qp = reinterpret_cast<const ks_u32x4*>(a.qb + (size_t)(q0 + (lane & 31)) * D) + (lane >> 5) + half * KH * 2;
#pragma unroll
            for (int i = 0; i < KH; ++i) fa[i] = __builtin_bit_cast(ks_bf16x8, qp[i * 2]);
        }
        // "used" here, so that hipcc waits for these loads here and not with a vmcnt(0) in front of the first MFMA of every step
#pragma unroll
        for (int i = 0; i < KH; ++i) asm volatile("" : "+v"(fa[i]));
    }
    if (half == 0 && lane < 32) {
        // conservative bound of the hot test: rows with acc >= sim_lo are looked at (a superset of `1 - acc <= tau` by less than 1e-6);
        // the exact test in the cold path decides
        const float tq = a.tau[q0 + lane];
        sim_s[pair * 32 + lane] = (1.0f - tq) - 4e-7f * (1.0f + __builtin_fabsf(tq));
    }

    const uint32_t ntiles = (a.slab_rows + KS_TROWS - 1) / KS_TROWS;
    const uint32_t slab_end = a.slab0 + a.slab_rows;
    const unsigned char* cbase = reinterpret_cast<const unsigned char*>(a.cb) + (size_t)a.slab0 * (D * 2);

    // LDS-DMA map: wave w issues requests w, w + 8, ...; lane l of request P fills slot 64 P + l of the step's pair image. Slot ->
    // (padded row rr of 64: rows 0-31 the lower half's piece, 32-63 the upper half's; 16-byte column c of 33).
    const bool full_wave = wave < KS_FULL_WAVES;
    constexpr uint32_t DIV_SHIFT = 18, DIV_MAGIC = ((1u << DIV_SHIFT) + KS_SLOTS_PER_ROW - 1) / KS_SLOTS_PER_ROW;
    static_assert((uint64_t)(KS_REQS * 64) * (DIV_MAGIC * (uint64_t)KS_SLOTS_PER_ROW - (1u << DIV_SHIFT)) < (1u << DIV_SHIFT),
                  "magic division must be exact for every slot of a step");
    auto slot_offset = [&](uint32_t P, uint32_t lane_o) -> uint32_t {
        const uint32_t slot = P * 64u + lane_o;
        const uint32_t rr = (slot * DIV_MAGIC) >> DIV_SHIFT;
        const uint32_t c = slot - rr * (uint32_t)KS_SLOTS_PER_ROW;
        return (rr & 31u) * (uint32_t)(D * 2) + (rr >> 5) * (uint32_t)D + c * 16u;   // row, K half (D bytes = D / 2 elements), column
    };
    constexpr bool CACHE_OFF = D <= 1024;            // per-request offsets in VGPRs where the fragments leave room
    uint32_t doff[CACHE_OFF ? KS_PPW : 1];
    if constexpr (CACHE_OFF) {
#pragma unroll
        for (int i = 0; i < KS_PPW; ++i) doff[i] = slot_offset((uint32_t)wave + 8u * (uint32_t)i, (uint32_t)lane);
    }
    auto dma_step = [&](uint32_t tile, uint32_t step, uint32_t buf_off) {
        const unsigned char* tbase = cbase + (size_t)tile * (KS_TROWS * D * 2) + step * (uint32_t)(KS_STEP_COLS * 2);   // wave-uniform
#pragma unroll
        for (int i = 0; i < KS_PPW; ++i) {
            if (i < KS_PPW - 1 || full_wave) {
                const uint32_t P = (uint32_t)wave + 8u * (uint32_t)i;
                uint32_t off;
                if constexpr (CACHE_OFF) {
                    off = doff[i];
                } else {
                    uint32_t lane_o = (uint32_t)lane;
                    asm volatile("" : "+v"(lane_o));      // recomputed per request: no per-request VGPRs live around the tile loop
                    off = slot_offset(P, lane_o);
                }
                __builtin_amdgcn_global_load_lds((ks_global_cvoid*)(tbase + off), (ks_lds_void*)(ks_smem + buf_off + P * 1024u), 16, 0, 0);
            }
        }
    };
    // this wave's requests still allowed in flight: the newest step's, or none
    auto dma_wait = [&](bool keep) {
        if (!keep) ks_wait_vmcnt<0>();
        else if (full_wave) ks_wait_vmcnt<KS_PPW>();
        else ks_wait_vmcnt<KS_PPW - 1>();
    };

    ks_f32x16 acc;
    const uint32_t smem_lds = (uint32_t)(size_t)(ks_lds_void*)ks_smem;
    const uint32_t lane_boff = (uint32_t)half * (uint32_t)KS_PIECE_B + (uint32_t)(lane & 31) * (uint32_t)KS_ROW_B + (uint32_t)(lane >> 5) * 16u;
    const uint32_t part_addr = smem_lds + (uint32_t)(KS_NRING * KS_PAIR_B) + (uint32_t)pair * 4096u + (uint32_t)lane * 16u;
    const uint32_t sim_addr = smem_lds + (uint32_t)(KS_NRING * KS_PAIR_B + KS_PART_B) + (uint32_t)(pair * 32 + 4 * (lane >> 5)) * 4u;
    // One step's K loop: fragment f + AHEAD is requested before MFMA f; the wait in front of MFMA f leaves at most
    // min(AHEAD, FPS - 1 - f) younger reads outstanding (LDS operations return in order). Every step is pinned (sched_barrier).
    auto mfma_step = [&](auto S, uint32_t baddr) {
        constexpr int s = decltype(S)::value;
        const ks_f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        ks_u32x4 fb[RING];
        ks_static_for<0, AHEAD>([&](auto F) {
            constexpr int f = decltype(F)::value;
            ks_u32x4(&fbr)[RING] = fb;
            const uint32_t ba = baddr;
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fbr[f % RING]) : "v"(ba), "n"(f * 32));
        });
        __builtin_amdgcn_s_setprio(1);
        __builtin_amdgcn_sched_barrier(0);
        ks_static_for<0, FPS>([&](auto F) {
            constexpr int f = decltype(F)::value;
            constexpr int g = f + AHEAD;
            ks_u32x4(&fbr)[RING] = fb;
            const uint32_t ba = baddr;
            if constexpr (g < FPS)
                asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fbr[g % RING]) : "v"(ba), "n"(g * 32));
            constexpr int younger = (FPS - 1 - f) < AHEAD ? (FPS - 1 - f) : AHEAD;
            asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(younger) : "memory");
            __builtin_amdgcn_sched_barrier(0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s * FPS + f], __builtin_bit_cast(ks_bf16x8, fbr[f % RING]),
                                                          (s == 0 && f == 0) ? zero16 : acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        });
        __builtin_amdgcn_s_setprio(0);
    };
    // Upper wave, behind its last step of a tile: the lane's 16 partials -> part[pair][quad][lane]. The nops cover the wait states
    // between the last MFMA's write of `acc` and an LDS instruction that reads it (hipcc does not look inside the statement).
    auto write_partials = [&]() {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
        ks_static_for<0, 4>([&](auto J) {
            constexpr int j = decltype(J)::value;
            const f32x4 v = {acc[4 * j], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3]};
            const uint32_t pa = part_addr;
            asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(pa), "v"(v), "n"(j * 1024) : "memory");
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    // Lower wave, behind that step's barrier: add the partner's partials and select. C/D layout of the 32x32 MFMA: column = lane & 31
    // (row of the tile), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (query of the pair).
    auto select_tile = [&](uint32_t tile) {
        f32x4 v4[4];
        ks_static_for<0, 4>([&](auto J) {
            constexpr int j = decltype(J)::value;
            f32x4(&vr)[4] = v4;
            const uint32_t pa = part_addr;
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(vr[j]) : "v"(pa), "n"(j * 1024) : "memory");
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += v4[r >> 2][r & 3];         // partial_lo + partial_hi: one more f32 rounding
        ks_static_for<0, 4>([&](auto J) {
            constexpr int j = decltype(J)::value;
            f32x4(&vr)[4] = v4;
            const uint32_t sa = sim_addr;
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(vr[j]) : "v"(sa), "n"(j * 32) : "memory");
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        // hot test: the sign of (acc - bound) pushed into a per-lane mask (1 = fails; a NaN may read as "passes": the exact test decides)
        unsigned fm = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) fm = __builtin_amdgcn_alignbit(fm, __float_as_uint(acc[r] - v4[r >> 2][r & 3]), 31u);
        const unsigned pm = ~fm & 0xFFFFu;                                 // bit 15 - r: accumulator r passes
        if (__ballot(pm != 0u) == 0ull) return;
        const uint32_t row = a.slab0 + tile * (uint32_t)KS_TROWS + (uint32_t)(lane & 31);
        // cold path: each lane walks its own passing bits — the accumulator picked by a four-level select tree on the bit's index
        // (registers cannot be indexed by a lane's value), then the exact test
        unsigned left = row < slab_end ? pm : 0u;
        while (left != 0u) {
            const unsigned r = 15u - (unsigned)__builtin_ctz(left);
            left &= left - 1u;
            float tsel[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) tsel[i] = acc[i];
#pragma unroll
            for (int bit = 0; bit < 4; ++bit) {
                const bool hi = (r >> bit) & 1u;
#pragma unroll
                for (int i = 0; i < (8 >> bit); ++i) tsel[i] = hi ? tsel[2 * i + 1] : tsel[2 * i];
            }
            const uint32_t q = q0 + (r & 3u) + 8u * (r >> 2) + 4u * ((uint32_t)lane >> 5);
            const float d = (1.0f - tsel[0]) + 0.0f;
            if (d <= a.tau[q]) {                                          // a NaN fails; padded queries have tau = -inf
                const uint32_t pos = atomicAdd(&a.cand_count[(size_t)q * CAND_COUNT_STRIDE], 1u);
                if (pos < a.cand_cap) a.cand[(size_t)q * a.cand_cap + pos] = make_key(d, a.row_base + row);
            }
        }
    };

    uint32_t t = bidx;                                                    // bidx < per_group <= ntiles
    dma_step(t, 0u, 0u);
    dma_step(t, 1u, (uint32_t)KS_PAIR_B);
    dma_wait(true);
    __builtin_amdgcn_s_barrier();                                         // also publishes sim_s
    asm volatile("" ::: "memory");
    uint32_t cur = 0;                                                     // ring index of the step being multiplied
    for (; t < ntiles; t += blocks_per_group) {
        ks_static_for<0, SPT>([&](auto S) {
            constexpr int s = decltype(S)::value;
            constexpr int s2 = (s + 2) % SPT, dj = (s + 2) / SPT;         // the step two ahead: of this tile or of the next
            const uint32_t tn = t + (uint32_t)dj * blocks_per_group;
            const bool issued = tn < ntiles;
            uint32_t nb = cur + 2u;
            nb = nb >= (uint32_t)KS_NRING ? nb - (uint32_t)KS_NRING : nb;
            // its buffer was read in the step before this one: every wave is past that step's barrier
            if (issued) dma_step(tn, (uint32_t)s2, nb * (uint32_t)KS_PAIR_B);
            mfma_step(S, smem_lds + cur * (uint32_t)KS_PAIR_B + lane_boff);
            dma_wait(issued);                                             // this wave's requests of the NEXT step have landed
            if constexpr (s == SPT - 1) { if (half == 1) write_partials(); }
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if constexpr (s == SPT - 1) { if (half == 0) select_tile(t); }
            cur = cur + 1u == (uint32_t)KS_NRING ? 0u : cur + 1u;
        });
    }
}

bool batch_ksplit_dims(uint32_t dims, int metric) { return metric != M_L2 && (dims == 1024u || dims == 1536u); }

void batch_ksplit_geometry(uint32_t nq_pad, uint32_t n_rows, uint32_t* groups, uint32_t* per_group) {
    const uint32_t ntiles = (n_rows + KS_TROWS - 1) / KS_TROWS;
    *groups = nq_pad / KS_QUERIES;
    uint32_t pg = *groups ? 256u / *groups : 1u;      // one persistent workgroup per CU in total
    if (pg < 1u) pg = 1u;
    if (pg > ntiles) pg = ntiles;
    *per_group = pg;
}

template <int D>
static hipError_t launch_ks(const GemmArgs& a, hipStream_t st) {
    uint32_t groups, per_group;
    batch_ksplit_geometry(a.nqt * 128u, a.slab_rows, &groups, &per_group);
    static std::atomic<uint64_t> configured{0};   // per device (ensure_dynamic_lds)
    const hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&batch_gemm_ks_kernel<D>), KS_SMEM, configured);
    if (e != hipSuccess) return e;
    launch_kernel((batch_gemm_ks_kernel<D>), dim3(groups * per_group), dim3(512), (uint32_t)KS_SMEM, st, a, per_group);
    return hipGetLastError();
}

hipError_t launch_batch_gemm_ks(const GemmArgs& a, int metric, hipStream_t st) {
    if (!batch_ksplit_dims(a.dims, metric) || a.dense != nullptr || a.nqt == 0u || a.slab_rows == 0u || a.cb == nullptr || a.tau == nullptr ||
        a.cand == nullptr || a.cand_count == nullptr || (a.qf == nullptr && a.qb == nullptr) || a.slab0 + a.slab_rows > a.n_rows)
        return hipErrorInvalidValue;
    return a.dims == 1024u ? launch_ks<1024>(a, st) : launch_ks<1536>(a, st);
}

}  // namespace wax
