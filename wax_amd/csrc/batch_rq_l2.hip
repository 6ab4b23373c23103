// batch_rq_l2.hip — the register-resident filtering GEMM for L2 stores at 384 and 768 dimensions: the filtering launch of the one-pass
// batched pipeline with GemmArgs::ksplit == BATCH_FILTER_RQ_L2 ("The register-resident L2 filter"; wax_hip_search_batch_l2,
// api_batch_l2.inc). The LDS-tiled batch_gemm_kernel<M_L2> is what every other L2 batch still runs.
//
//   batch_gemm_rq_l2_kernel<D>  512 threads, 8 waves, two per SIMD. Each wave keeps its 32 queries x D resident as
//                               v_mfma_f32_32x32x16_bf16 A fragments (96 / 192 VGPRs), read from the prep kernel's fragment-ordered copy
//                               (GemmArgs::qf). nq_pad / 256 query groups of 256 / groups persistent workgroups; workgroup bidx of a
//                               group walks the tiles bidx, bidx + per_group, ... of RqGeom<D>'s shape (64 rows and a ring of two at
//                               384-d, 32 rows and a ring of three at 768-d). Fixed shares throughout: no tail pool, no pace gate.
//   data movement               batch_gemm_rq_kernel's (batch_rq.h): tile images by LDS-DMA in 1-KB pieces at the row stride 2 D + 16,
//                               un-clamped inside BATCH_MIRROR_SLACK_ROWS; B fragments by hand-counted ds_read_b128; one workgroup
//                               barrier per tile; waves 0-3 multiply and then select, waves 4-7 select the previous tile and then
//                               multiply; with three buffers the early waves request behind their K loop.
//   the norm slice              ||v||^2 of a tile's rows travels with the tile: wave 7 (which carries one piece less than wave 0) adds ONE
//                               4-byte-per-lane LDS-DMA request per tile, lane l fetching v_n2[min(row0 + l, n_rows - 1)] into
//                               norm[buffer][l]; its vmcnt accounting grows by one, to wave 0's. The index is clamped because
//                               BatchMirror::d_vn2 is allocated with exactly `capacity` floats (batch_host.inc, ensure_mirror: the slack
//                               rows belong to the bf16 mirror alone) — rows >= slab_end are masked by the selection anyway. The area is
//                               [NBUF][64] floats at both dimensions: a request is 64 lanes wide, at 768-d the upper 32 words of a slot
//                               are written and never read. A slot is rewritten by the request issued one tile barrier after its last
//                               reader: every wave reads its lane's norm (ds_read_b32, inline) behind the K loop of the tile.
//   selection                   batch_gemm_kernel<M_L2>'s contract: d = (qq + vn2 - 2.0f * dot) + 0.0f <= tau[q] for rows < slab_end (a
//                               NaN fails), key make_key(d, row_base + row), appended at atomicAdd(&cand_count[q * CAND_COUNT_STRIDE], 1)
//                               and stored only below cand_cap; the count is never clamped. That is the cold path, and it alone decides.
//
// The hot test. In a 32 x 32 accumulator lane l holds ONE store row (column l & 31) and 16 queries, so the row's norm is one value per
// lane and block. With b_q = 0.5 (qq - tau_q) the exact condition d <= tau reads acc - 0.5 vn2 >= b_q: per accumulator one v_fma
// (t = fma(-0.5, vn2, acc): the product is exact, one rounding), one subtraction t - lo_q and the funnel shift that gathers the sign —
// one VALU operation more than the cosine kernel's — and one ballot per tile.
//   Slack. lo_q = 0.5 (qq - tau) - 1e-6 (qq + |tau|) - 1e-30. Claim: for finite tau every pair the cold test admits passes the hot test.
//   With u = 2^-24, A = |acc| and M = qq + vn2 + 2 A: the cold d is within 2 u M of S = qq + vn2 - 2 acc (two roundings, each of a
//   value at most M), so an admitted pair has S <= tau + 2 u M, i.e. the real H = acc - vn2 / 2 - (qq - tau) / 2 >= -u M. The computed t
//   is below acc - vn2 / 2 by at most u (A + vn2 / 2), the computed 0.5 (qq - tau) above the real one by at most 0.5 u |qq - tau|, and the
//   final subtraction has the sign of its exact operands. So the hot test passes if the slack is at least
//   u (M + A + vn2 / 2 + |qq - tau| / 2). The row's terms are bounded through the admission itself: A <= ||q~|| ||v~|| (1 + D u) <=
//   1.01 sqrt(qq vn2) (bf16 rounding moves a norm by at most 2^-8 relative, the f32 norms by D u), hence A <= 0.505 (qq + vn2), and
//   S <= tau + 2 u M gives (sqrt(vn2) - 1.01 sqrt(qq))^2 <= tau+ + 0.0201 qq + 2 u M, hence vn2 <= 2.09 qq + 2 tau+ (tau+ = max(tau, 0)).
//   Together: slack / u <= 3.02 qq + 3.02 vn2 + 0.5 |tau| <= 9.4 qq + 6.6 |tau|, and 1e-6 = 16.8 u covers it 1.7 times over — in units
//   of the rounding of ||q||^2 + ||v||^2 + 2 |q.v|, not of tau alone: at tau -> 0 (a planted duplicate) the slack stays 1e-6 qq.
//   tau = +inf (prep's initial value; pick_tau found no threshold): lo = -inf, and the lane's mask is forced to "passes" for such
//   queries (`force`, one OR per block and tile), because t - lo may be NaN there (a row with non-finite elements) — the cold test then
//   admits what the LDS-tiled kernel admits, and the unclamped count sends the query to the exact ladder when the list overflows.
//   tau = -inf (padded queries): lo = +inf, every difference is -inf or NaN; the cold test `d <= -inf` admits nothing.
//   NaN rows (vn2 or acc NaN): the difference is NaN and may read either way; the cold test fails a NaN. For finite tau an admitted
//   pair has finite qq + vn2 and acc, so none of the arithmetic above meets an infinity.
//
// Exactness. The accumulators start at ZERO and a product is one chain of D / 16 MFMAs, as in the cosine kernel: prep's eps for L2
// (2 dot_err + 4e-6 (1 + ss)) bounds |d - exact| for exactly this form and is shared with searchBatch. (Seeding the accumulators with
// -vn2 / 2 would save the fma and put an accumulation that starts at the norm outside that bound.)
// No LDS access the compiler can see sits inside the tile loop; every list, count and key is written with vector stores.
#include "batch_rq.h"
#include "kernels.h"
#include "row_math.h"

namespace wax {

constexpr int RQL2_QUERIES = (int)BATCH_GROUP_QUERIES;   // queries per workgroup: eight waves of 32
constexpr int RQL2_NORM_B = 64 * 4;                      // one norm slot: a 64-lane request of 4 bytes
constexpr int RQL2_NORM_WAVE = 7;                        // the wave that requests the norm slice
template <int D>
constexpr size_t rql2_smem() {
    using G = RqGeom<D>;
    return (size_t)G::NBUF * RqTile<D, G::TROWS>::BUF_B + (size_t)G::NBUF * RQL2_NORM_B + 8 * 32 * 4;   // tile ring, norm slots, bounds
}

template <int D, bool NT>
__global__ __launch_bounds__(512, 2) void batch_gemm_rq_l2_kernel(GemmArgs a, uint32_t blocks_per_group) {
    using G = RqGeom<D>;
    constexpr int TROWS = G::TROWS, NBUF = G::NBUF, AHEAD = G::AHEAD;
    using T = RqTile<D, TROWS>;
    constexpr int KS = T::KS, RB = T::RB, ROW_B = T::ROW_B, BUF_B = T::BUF_B, PPW = T::PPW, FULL_WAVES = T::FULL_WAVES;
    constexpr int PRE = NBUF - 1;                    // tiles requested ahead of the one being read
    constexpr int NORM_OFF = NBUF * BUF_B, BOUND_OFF = NORM_OFF + NBUF * RQL2_NORM_B;
    static_assert(FULL_WAVES <= RQL2_NORM_WAVE, "the norm wave carries PPW - 1 pieces: with the norm request it counts PPW, like a full wave");
    static_assert(TROWS <= 64, "one 64-lane request covers a tile's norms");
    static_assert(rql2_smem<D>() <= 160 * 1024, "LDS budget of one CU");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* lo_s = reinterpret_cast<float*>(smem + BOUND_OFF);    // [8][32] conservative bounds of the hot test

    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform
    const uint32_t group = blockIdx.x / blocks_per_group;        // 256 queries per group
    const uint32_t bidx = blockIdx.x % blocks_per_group;
    const uint32_t q0 = group * (uint32_t)RQL2_QUERIES + (uint32_t)wave * 32u;   // this wave's 32 queries

    // A fragments: lane l holds query (l & 31), k = 16 ks + 8 (l >> 5) .. + 7
    bf16x8 fa[KS];
    {
        if (a.qf != nullptr) {   // fragment order: one contiguous 1-KB run per k-step
            const u32x4* qp = reinterpret_cast<const u32x4*>(a.qf) + (size_t)(q0 >> 5) * (KS * 64) + lane;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) fa[ks] = __builtin_bit_cast(bf16x8, qp[ks * 64]);
        } else {
            const u32x4* qp = reinterpret_cast<const u32x4*>(a.qb + (size_t)(q0 + (lane & 31)) * D) + (lane >> 5);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) fa[ks] = __builtin_bit_cast(bf16x8, qp[ks * 2]);
        }
        // "used" here, so that hipcc waits for these loads here and not with a vmcnt(0) in front of the first MFMA of every tile
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(fa[ks]));
    }
    if (lane < 32) {   // the hot test's bound (header: "Slack"); a padded query (tau = -inf) gets +inf, not inf - inf
        const float tq = a.tau[q0 + lane], qq = a.q_n2[q0 + lane];
        const float lo = 0.5f * (qq - tq) - 1e-6f * (qq + __builtin_fabsf(tq)) - 1e-30f;
        lo_s[wave * 32 + lane] = tq == -__builtin_inff() ? __builtin_inff() : lo;
    }

    const uint32_t ntiles = (a.slab_rows + TROWS - 1) / TROWS;
    const uint32_t slab_end = a.slab0 + a.slab_rows;
    const uint32_t last_row = a.n_rows - 1u;
    const unsigned char* cbase = reinterpret_cast<const unsigned char*>(a.cb);

    // LDS-DMA map (batch_rq.h): wave w moves pieces w, w + 8, ... of a tile; wave 7 also its norm slice
    const bool full_wave = wave < FULL_WAVES;
    const bool norm_wave = wave == RQL2_NORM_WAVE;
    constexpr bool CACHE_OFF = D <= 512;             // per-piece offsets in VGPRs: a request is ONE instruction
    uint32_t doff[CACHE_OFF ? PPW : 1];
    if (CACHE_OFF) {
#pragma unroll
        for (int i = 0; i < PPW; ++i) doff[i] = T::slot_offset(((uint32_t)wave + 8u * (uint32_t)i) * 64u + (uint32_t)lane);
    }
    auto dma_tile = [&](uint32_t tile, uint32_t buf) {
        const uint32_t row0 = a.slab0 + tile * TROWS;
        const unsigned char* tbase = cbase + (size_t)row0 * (D * 2);   // wave-uniform
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            if (i < PPW - 1 || full_wave) {
                const uint32_t P = (uint32_t)wave + 8u * (uint32_t)i;
                uint32_t off;
                if constexpr (CACHE_OFF) {
                    off = doff[i];
                } else {
                    uint32_t lane_o = (uint32_t)lane;
                    asm volatile("" : "+v"(lane_o));      // recomputed per piece: no per-piece VGPRs live around the tile loop
                    off = T::slot_offset(P * 64u + lane_o);
                }
                // NT (one query group: every tile is read exactly once): non-temporal requests
                __builtin_amdgcn_global_load_lds((global_cvoid*)(tbase + off), (lds_void*)(smem + buf * (uint32_t)BUF_B + P * 1024u), 16, 0, NT ? 2 : 0);
            }
        }
        if (norm_wave) {
            uint32_t r = row0 + (uint32_t)lane;
            r = r < last_row ? r : last_row;              // d_vn2 has no slack rows behind it
            __builtin_amdgcn_global_load_lds((global_cvoid*)(a.v_n2 + r), (lds_void*)(smem + NORM_OFF + buf * (uint32_t)RQL2_NORM_B), 4, 0, 0);
        }
    };
    // this wave's DMA requests still allowed in flight: PRE - 1 whole tiles (PPW requests each for wave 0 and the norm wave), or none
    const bool count_full = full_wave || norm_wave;
    auto dma_wait = [&](bool keep) {
        if (!keep) wait_vmcnt<0>();
        else if (count_full) wait_vmcnt<(PRE - 1) * PPW>();
        else wait_vmcnt<(PRE - 1) * (PPW - 1)>();
    };

    f32x16 acc[RB];
    float vn2[RB];                                   // the lane's row norm per block of the tile in `acc`
    const uint32_t smem_lds = (uint32_t)(size_t)(lds_void*)smem;
    const uint32_t lane_boff = (uint32_t)(lane & 31) * (uint32_t)ROW_B + (uint32_t)(lane >> 5) * 16u;
    const uint32_t norm_addr = smem_lds + (uint32_t)NORM_OFF + (uint32_t)(lane & 31) * 4u;
    const uint32_t lo_addr = smem_lds + (uint32_t)BOUND_OFF + (uint32_t)(wave * 32 + 4 * (lane >> 5)) * 4u;
    // the lane's norms of the tile in ring slot `buf`, behind the tile's K loop (the round trip overlaps the last MFMAs' passes; the wait
    // sits inside the statement, so the registers are valid wherever the compiler reads them)
    auto read_norms = [&](uint32_t buf) {
        static_for<0, RB>([&](auto B) {
            constexpr int b = decltype(B)::value;
            float(&vr)[RB] = vn2;
            const uint32_t na = norm_addr + buf * (uint32_t)RQL2_NORM_B;
            asm volatile("ds_read_b32 %0, %1 offset:%2\n\ts_waitcnt lgkmcnt(0)" : "=v"(vr[b]) : "v"(na), "n"(b * 128) : "memory");
        });
    };
    // the lane's sixteen bounds (queries (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the wave): in registers where they fit, else re-read per tile
    constexpr bool BOUNDS_REGS = D <= 512;
    f32x4 lo_keep[4];
    unsigned force = 0u;                             // bit 15 - r: query r has tau = +inf — the hot test admits every row
    auto read_bounds = [&](f32x4(&lor)[4]) {
        static_for<0, 4>([&](auto J) {
            constexpr int j = decltype(J)::value;
            f32x4(&l4)[4] = lor;
            const uint32_t la = lo_addr;
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(l4[j]) : "v"(la), "n"(j * 32));
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    // Fused selection on the tile in `acc`. C/D layout of the 32x32 MFMA: column = lane & 31 (row of the block), row =
    // (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (query of the wave). A wave's 32 queries are its own.
    auto select_tile = [&](uint32_t tile) {
        f32x4 lo[4];
        if constexpr (BOUNDS_REGS) {
#pragma unroll
            for (int j = 0; j < 4; ++j) lo[j] = lo_keep[j];
        } else {
            read_bounds(lo);
        }
        unsigned pm[RB], anyp = 0u;
#pragma unroll
        for (int b = 0; b < RB; ++b) {
            unsigned fm = 0u;                        // 1 = fails; a NaN may read as "passes": the cold test decides
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float t = __builtin_fmaf(-0.5f, vn2[b], acc[b][r]);
                fm = __builtin_amdgcn_alignbit(fm, __float_as_uint(t - lo[r >> 2][r & 3]), 31u);
            }
            pm[b] = (~fm | force) & 0xFFFFu;         // bit 15 - r: accumulator r passes
            anyp |= pm[b];
        }
        if (__ballot(anyp != 0u) == 0ull) return;
        // cold path: each lane walks its own passing bits — the accumulator picked by a four-level select tree on the bit's index
        // (registers cannot be indexed by a lane's value), then the LDS-tiled kernel's test and append, to the letter
#pragma unroll
        for (int b = 0; b < RB; ++b) {
            const uint32_t row = a.slab0 + tile * TROWS + (uint32_t)b * 32u + (uint32_t)(lane & 31);
            unsigned left = row < slab_end ? pm[b] : 0u;
            while (left != 0u) {
                const unsigned r = 15u - (unsigned)__builtin_ctz(left);
                left &= left - 1u;
                float tsel[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) tsel[i] = acc[b][i];
#pragma unroll
                for (int bit = 0; bit < 4; ++bit) {
                    const bool hi = (r >> bit) & 1u;
#pragma unroll
                    for (int i = 0; i < (8 >> bit); ++i) tsel[i] = hi ? tsel[2 * i + 1] : tsel[2 * i];
                }
                const uint32_t q = q0 + (r & 3u) + 8u * (r >> 2) + 4u * ((uint32_t)lane >> 5);
                const float dot = tsel[0];
                float d = a.q_n2[q] + vn2[b] - 2.0f * dot;
                d += 0.0f;
                if (d <= a.tau[q]) {                                      // a NaN fails; padded queries have tau = -inf
                    const uint32_t pos = atomicAdd(&a.cand_count[(size_t)q * CAND_COUNT_STRIDE], 1u);
                    if (pos < a.cand_cap) a.cand[(size_t)q * a.cand_cap + pos] = make_key(d, a.row_base + row);
                }
            }
        }
    };

    {   // prologue: the first PRE tiles of this workgroup (bidx < per_group <= ntiles)
        bool all = true;
#pragma unroll
        for (int i = 0; i < PRE; ++i) {
            const uint32_t ti = bidx + (uint32_t)i * blocks_per_group;
            if (ti < ntiles) dma_tile(ti, (uint32_t)i); else all = false;
        }
        dma_wait(all);
        __builtin_amdgcn_s_barrier();                             // also publishes lo_s
        asm volatile("" ::: "memory");
    }
    {
        read_bounds(lo_keep);
#pragma unroll
        for (int r = 0; r < 16; ++r) force = (force << 1) | (lo_keep[r >> 2][r & 3] == -__builtin_inff() ? 1u : 0u);
    }
    const bool late = wave >= 4;
    // three tile buffers: an EARLY wave starts its K loop at once and requests behind it (batch_gemm_rq_kernel, round 6)
    constexpr bool EARLY_AFTER = NBUF >= 3;
    uint32_t cur = 0, t_prev = 0;
    bool first = true;
    for (uint32_t t = bidx; t < ntiles; t += blocks_per_group) {
        const uint32_t tn = t + (uint32_t)PRE * blocks_per_group;
        const bool issued = tn < ntiles;
        uint32_t pre = cur + (uint32_t)PRE;
        pre = pre >= (uint32_t)NBUF ? pre - (uint32_t)NBUF : pre;
        if (late && !first) select_tile(t_prev);
        // every wave is past the previous tile's barrier: the buffer and the norm slot tile tn goes to have been read
        if (!(EARLY_AFTER && !late) && issued) dma_tile(tn, pre);
        rq_mfma_tile<KS, RB, ROW_B, AHEAD>(fa, acc, smem_lds + cur * (uint32_t)BUF_B + lane_boff);
        read_norms(cur);                                          // (a late wave selects this tile at the top of the next iteration)
        if (EARLY_AFTER && !late && issued) dma_tile(tn, pre);
        // this wave's requests of the NEXT tile have landed (the barrier joins the waves); the PRE - 1 younger tiles stay in flight
        dma_wait(issued);
        if (!late) select_tile(t);
        t_prev = t;
        first = false;
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        cur = cur + 1u == (uint32_t)NBUF ? 0u : cur + 1u;
    }
    if (late && !first) select_tile(t_prev);
}

bool batch_rq_l2_dims(uint32_t dims, int metric) { return metric == M_L2 && (dims == 384u || dims == 768u); }

void batch_rq_l2_geometry(uint32_t dims, uint32_t nq_pad, uint32_t n_rows, uint32_t* groups, uint32_t* per_group, uint32_t* tile_rows) {
    const uint32_t tr = dims == 768u ? (uint32_t)RqGeom<768>::TROWS : (uint32_t)RqGeom<384>::TROWS;
    const uint32_t ntiles = (n_rows + tr - 1) / tr;
    *groups = nq_pad / (uint32_t)RQL2_QUERIES;
    uint32_t pg = *groups ? 256u / *groups : 1u;      // one persistent workgroup per CU in total
    if (pg < 1u) pg = 1u;
    if (pg > ntiles) pg = ntiles;
    *per_group = pg;
    *tile_rows = tr;
}

template <int D, bool NT>
static hipError_t launch_rql2(const GemmArgs& a, uint32_t groups, uint32_t per_group, hipStream_t st) {
    static std::atomic<uint64_t> configured{0};   // per device (ensure_dynamic_lds)
    const hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&batch_gemm_rq_l2_kernel<D, NT>), rql2_smem<D>(), configured);
    if (e != hipSuccess) return e;
    launch_kernel((batch_gemm_rq_l2_kernel<D, NT>), dim3(groups * per_group), dim3(512), (uint32_t)rql2_smem<D>(), st, a, per_group);
    return hipGetLastError();
}

hipError_t launch_batch_gemm_rq_l2(const GemmArgs& a, int metric, hipStream_t st) {
    if (!batch_rq_l2_dims(a.dims, metric) || a.dense != nullptr || a.nqt == 0u || (a.nqt & 1u) != 0u || a.slab_rows == 0u || a.n_rows == 0u ||
        a.cb == nullptr || a.tau == nullptr || a.q_n2 == nullptr || a.v_n2 == nullptr || a.cand == nullptr || a.cand_count == nullptr ||
        (a.qf == nullptr && a.qb == nullptr) || a.slab0 + a.slab_rows > a.n_rows)
        return hipErrorInvalidValue;
    uint32_t groups, per_group, tile_rows;
    batch_rq_l2_geometry(a.dims, a.nqt * 128u, a.slab_rows, &groups, &per_group, &tile_rows);
    // one query group: every tile is requested exactly once -> non-temporal requests (batch_gemm_rq_kernel's rule)
    if (a.dims == 384u) return groups == 1u ? launch_rql2<384, true>(a, groups, per_group, st) : launch_rql2<384, false>(a, groups, per_group, st);
    return groups == 1u ? launch_rql2<768, true>(a, groups, per_group, st) : launch_rql2<768, false>(a, groups, per_group, st);
}

}  // namespace wax
