// batch_rq.h — what the register-resident filtering GEMMs share (device side; included by batch.hip and batch_rq_l2.hip only):
// batch_gemm_rq_kernel (cosine / dot) and batch_gemm_rq_l2_kernel (L2) keep a wave's 32 queries x D as MFMA A fragments and stream
// the bf16 mirror through a ring of padded tile images in LDS. Both use the geometry table, the slot map of the LDS-DMA requests and
// the K loop below; what differs between them — the selection, the barrier forms, the sampling launch, the norm slice — stays in its unit.
#pragma once
#include <type_traits>

#include "kernels.h"
#include "row_math.h"

namespace wax {

// Compile-time loop: f(std::integral_constant<int, I>{}) for I in [I0, N) — the index is a constant expression inside
// f (inline-asm immediates need one; an unrolled loop variable is not).
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
typedef __attribute__((address_space(3))) unsigned int lds_u32;
typedef __attribute__((address_space(3))) float lds_f32;
typedef __attribute__((address_space(3))) f32x4 lds_f32x4;
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void global_cvoid;

template <int N>
__device__ inline void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// Per-dimension geometry of the rq kernels: rows per tile (what the one-pass planner calls a tile), LDS tile buffers, read-ahead.
// D * TROWS is 16 - 32 K elements (32 - 64 MFMAs per wave and tile); three buffers where they fit beside the neighbouring batch's
// small kernels (a workgroup of ~100 KB leaves them a third of the CU's LDS; 150 KB does not: measured in round 3 and again in
// round 5 at D = 384, where two buffers lose nothing), except at D = 768 where a 32-row tile is already 48.5 KB and the third
// buffer is what lets a request stay in flight across a tile.
// (Round 6, D = 384: 96-row tiles — 2 x 75 KB — cut 7.6 % of the cycles per row and 4 % of the Q = 1 024 kernel, but a workgroup
// that fills the CU's LDS keeps the neighbouring batches' small kernels off it: pipelined 256-query batches +2 %, dense
// neighbourhoods +6 %. 64 rows stay: profiles/r06/g_*.)
// (Round 6, D = 384 with three buffers + the early waves requesting behind their K loop: +5 % cycles per tile, pipelined batches +4 ... 7 %.)
template <int D> struct RqGeom;
template <> struct RqGeom<128> { static constexpr int TROWS = 128, NBUF = 3, AHEAD = 3; };
template <> struct RqGeom<256> { static constexpr int TROWS = 64, NBUF = 3, AHEAD = 3; };
template <> struct RqGeom<384> { static constexpr int TROWS = 64, NBUF = 2, AHEAD = 3; };
template <> struct RqGeom<512> { static constexpr int TROWS = 64, NBUF = 2, AHEAD = 3; };
template <> struct RqGeom<768> { static constexpr int TROWS = 32, NBUF = 3, AHEAD = 3; };

// The padded tile image and its LDS-DMA map. A tile of TROWS rows lies in LDS at the row stride 2 D + 16 bytes (conflict-free
// ds_read_b128: (ROW_B / 4) % 64 == 4), cut into 1-KB pieces: wave w moves pieces w, w + 8, ...; lane l of piece P fills 16-byte slot
// 64 P + l. Slot -> global offset from the tile's first byte is 16 (slot - slot / SLOTS_PER_ROW), with no clamps: a pad slot fetches the
// first bytes of the next row, the slack behind the image the row after the tile, a tile that runs past the store whatever the mirror
// holds there — all inside the mirror's allocation (capacity + BATCH_MIRROR_SLACK_ROWS) and never used.
template <int D, int TROWS>
struct RqTile {
    static constexpr int KS = D / 16;                       // MFMA k-steps
    static constexpr int RB = TROWS / 32;                   // 32-row blocks per tile = accumulators per wave
    static constexpr int ROW_B = D * 2 + 16;                // LDS row stride (bytes)
    static constexpr int SEG_PER_ROW = D * 2 / 16;          // 16-byte segments per row
    static constexpr int SLOTS_PER_ROW = ROW_B / 16;        // 16-byte slots per padded row
    static constexpr int IMG_B = TROWS * ROW_B;             // padded tile image
    static constexpr int PIECES = (IMG_B + 1023) / 1024;    // 1-KB DMA pieces per tile
    static constexpr int BUF_B = PIECES * 1024;             // buffer stride (the image + slack for the last piece)
    static constexpr int PPW = (PIECES + 7) / 8;            // pieces per wave
    static constexpr int FULL_WAVES = PIECES % 8 == 0 ? 8 : PIECES % 8;   // waves below this index carry PPW pieces, the others PPW - 1
    static constexpr uint32_t DIV_SHIFT = 18, DIV_MAGIC = ((1u << DIV_SHIFT) + SLOTS_PER_ROW - 1) / SLOTS_PER_ROW;
    static_assert(TROWS % 32 == 0 && RB >= 1 && RB <= 4, "tile = 1..4 MFMA row blocks");
    static_assert(TROWS + 2 <= (int)BATCH_MIRROR_SLACK_ROWS, "the un-clamped requests of the last tile stay inside the mirror's slack rows");
    static_assert(D % 64 == 0 && (ROW_B / 4) % 64 == 4, "row stride must keep ds_read_b128 conflict-free");
    static_assert((RB - 1) * 32 * ROW_B + (KS - 1) * 32 < 65536, "ds_read offset field");
    static_assert((uint64_t)(PIECES * 64) * (DIV_MAGIC * (uint64_t)SLOTS_PER_ROW - (1u << DIV_SHIFT)) < (1u << DIV_SHIFT),
                  "magic division must be exact for every slot of a tile");
    // global byte offset (from the tile's first byte) that slot `slot` of the image is filled from
    static __device__ __forceinline__ uint32_t slot_offset(uint32_t slot) { return (slot - ((slot * DIV_MAGIC) >> DIV_SHIFT)) * 16u; }
};

// The K loop of one tile: acc[rb] = sum over k-steps of fa[ks] x (rows 32 rb .. + 31 of the image at LDS address baddr - the lane's
// own offset (lane & 31) * ROW_B + (lane >> 5) * 16 included), ONE chain of D / 16 MFMAs per accumulator starting from zero.
// B fragments are read by inline-asm ds_read_b128 with hand-counted lgkmcnt waits, so that no LDS access of the loop is visible to
// hipcc's waitcnt pass (which would drain the LDS-DMA queue in front of it). Fragment f + AHEAD is requested before MFMA f; the wait
// in front of MFMA f leaves at most min(AHEAD, NF - 1 - f) younger reads outstanding — LDS operations return in order, so fragment f
// and every LDS read the caller issued before the loop have landed. Every step is pinned (sched_barrier): hipcc otherwise hoists an
// MFMA over the asm wait it depends on. s_setprio 1 lets the multiplying wave win issue arbitration against its selecting partner.
template <int KS, int RB, int ROW_B, int AHEAD>
__device__ __forceinline__ void rq_mfma_tile(const bf16x8 (&fa)[KS], f32x16 (&acc)[RB], uint32_t baddr) {
    constexpr int NF = KS * RB;                      // B fragments (= MFMAs) per wave and tile; fragment f = (k-step f / RB, block f % RB)
    constexpr int RING = AHEAD + 1;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    u32x4 fb[RING];
    static_for<0, (AHEAD < NF ? AHEAD : NF)>([&](auto F) {
        constexpr int f = decltype(F)::value;
        u32x4(&fbr)[RING] = fb;                  // (asm operands alone do not make a generic lambda capture)
        const uint32_t ba = baddr;
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fbr[f % RING]) : "v"(ba), "n"((f % RB) * 32 * ROW_B + (f / RB) * 32));
    });
    __builtin_amdgcn_s_setprio(1);
    __builtin_amdgcn_sched_barrier(0);
    static_for<0, NF>([&](auto F) {
        constexpr int f = decltype(F)::value;
        constexpr int g = f + AHEAD;
        u32x4(&fbr)[RING] = fb;
        const uint32_t ba = baddr;
        if constexpr (g < NF)
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fbr[g % RING]) : "v"(ba), "n"((g % RB) * 32 * ROW_B + (g / RB) * 32));
        constexpr int younger = (NF - 1 - f) < AHEAD ? (NF - 1 - f) : AHEAD;
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(younger) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        constexpr int ks = f / RB, rb = f % RB;
        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks], __builtin_bit_cast(bf16x8, fbr[f % RING]), ks == 0 ? zero16 : acc[rb], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    });
    __builtin_amdgcn_s_setprio(0);
}

}  // namespace wax
