// multiscan_body.inc — the body of scan_multi_kernel / scan_multi_pooled_kernel (multiscan.hip includes it once per kernel; not compiled
// alone). In scope: the template arguments D4, GROUP, METRIC, CAP; constexpr bool LISTED, POOLED, MASKED; `a` (ScanMultiArgs); `pool`.
// MASKED (the pooled form of wax_hip_search_many_predicate only): a group may carry a row bitmap, and a row is offered only where its
// bit is set. Everything under `if constexpr (MASKED)` is absent from the other kernels, whose instructions stay as they were.
    constexpr int LOADS = D4 / GROUP;
    constexpr int RPW = WAVE / GROUP;
    constexpr int RPC = RPW * MS_U;
    constexpr int LEVELS = GROUP == 64 ? 6 : (GROUP == 32 ? 5 : 4);
    constexpr int OUT = MS_M >> LEVELS;          // complete sums per lane per chunk: 4 / 2 / 1
    static_assert(D4 % GROUP == 0 && (GROUP == 16 || GROUP == 32 || GROUP == 64), "GROUP");
    static_assert((RPC & (RPC - 1)) == 0 && RPC <= 32, "a chunk's bits must sit inside one bitmap word");
    static_assert(!MASKED || POOLED, "only the many-stores form has a masked kernel");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t nq = a.nq, n = a.n_rows, wg = blockIdx.x, nwg = gridDim.x, part0 = 0, row_base = a.row_base;
    const uint32_t* qlist = a.qlist;
    const float* qnorm = a.q_norm;
    const float* store = a.store;
    const uint32_t* __restrict__ rows = nullptr;
    const uint32_t* __restrict__ mask = nullptr;   // MASKED: the group's row bitmap (null: every row may be offered)
    if constexpr (LISTED) {
        const GatherGroup G = a.groups[a.item_group[blockIdx.x]];
        nq = G.nq; n = a.row_counts[G.count_slot]; wg = blockIdx.x - G.item0; nwg = G.n_items; part0 = G.part_off;
        qlist = a.qlist + G.q0; qnorm = a.q_norm + G.q0; rows = a.rows + G.row_off;
    }
    if constexpr (POOLED) {
        const PoolGroup G = pool[a.item_group[blockIdx.x]];
        nq = G.nq; n = G.n_rows; wg = blockIdx.x - G.item0; nwg = G.n_items; part0 = G.part_off;
        qlist = a.qlist + G.q0; qnorm = a.q_norm + G.q0; store = G.store; row_base = G.row_base;
        if constexpr (MASKED) mask = G.bitmap;
    }
    // partial list of query slot qi of this workgroup: [nq][grid][k] (full store) / [part_off + qi * n_items + wg] (listed)
    auto partial_of = [&](uint32_t qi) -> int64_t* {
        return a.partials + ((size_t)part0 + (size_t)qi * nwg + wg) * (size_t)a.k;
    };
    f32x4* qs = reinterpret_cast<f32x4*>(smem);                                            // [16][D4] (slots >= nq: zeros)
    int64_t* lists = reinterpret_cast<int64_t*>(smem + (size_t)MS_NQ * D4 * 16);           // [SCAN_WAVES][16][CAP]
    MsState* state = reinterpret_cast<MsState*>(lists + (size_t)SCAN_WAVES * MS_NQ * CAP);  // [SCAN_WAVES][16]
    float* qn_s = reinterpret_cast<float*>(state + SCAN_WAVES * MS_NQ);                     // [16]
    int* counts = reinterpret_cast<int*>(qn_s + MS_NQ);                                     // [16][SCAN_WAVES]

    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const int sub = lane / GROUP;
    const int gl = lane % GROUP;
    const int k = a.k;
    if constexpr (LISTED || POOLED) {
        // a share beyond the list's device-side count (the grid was sized by an upper bound): empty partial lists
        if (wg * (uint32_t)SCAN_WAVES >= (n + RPC - 1) / RPC) {
            for (uint32_t i = threadIdx.x; i < nq * (uint32_t)k; i += SCAN_THREADS) partial_of(i / (uint32_t)k)[i % (uint32_t)k] = KEY_PAD;
            return;
        }
    }

    for (uint32_t i = threadIdx.x; i < (uint32_t)MS_NQ * (uint32_t)D4; i += SCAN_THREADS) {
        const uint32_t qi = i / (uint32_t)D4, c = i - qi * (uint32_t)D4;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        qs[i] = qi < nq ? reinterpret_cast<const f32x4*>(a.queries)[(size_t)qlist[qi] * D4 + c] : zero;
    }
    if (threadIdx.x < MS_NQ) qn_s[threadIdx.x] = threadIdx.x < nq ? qnorm[threadIdx.x] : 0.f;
    for (uint32_t i = threadIdx.x; i < SCAN_WAVES * MS_NQ; i += SCAN_THREADS) { state[i].tau = KEY_PAD; state[i].cnt = 0; }
    __syncthreads();

    const f32x4* __restrict__ store4 = reinterpret_cast<const f32x4*>(store);
    int64_t* my_lists = lists + (size_t)wave * MS_NQ * CAP;
    MsState* my_state = state + (size_t)wave * MS_NQ;
    const lds_f32x4m* qs_l = (const lds_f32x4m*)qs + gl;

    // the lane's selection bits and its query
    const int b0 = lane & 1, b1 = (lane >> 1) & 1, b2 = (lane >> 2) & 1, b3 = (lane >> 3) & 1, b4 = (lane >> 4) & 1, b5 = (lane >> 5) & 1;
    const bool s1 = (b0 ^ b2) != 0, s2 = (b1 ^ b2) != 0, s3 = (b2 ^ b3) != 0, s4 = b3 != 0;
    const int q_lane = (s1 ? 1 : 0) | (s2 ? 2 : 0) | (s3 ? 4 : 0) | (s4 ? 8 : 0);
    const bool q_live = (uint32_t)q_lane < nq;
    const float qn_lane = qn_s[q_lane];
    int64_t tau_lane = KEY_PAD;                              // this wave's threshold for q_lane (kept current by the insert path)
    const int last_of_group = (lane & ~(GROUP - 1)) | (GROUP - 1);

    const uint32_t nchunks = (n + RPC - 1) / RPC;
    const uint32_t gwave = wg * SCAN_WAVES + wave;
    const uint32_t nwaves = nwg * SCAN_WAVES;

    // The rows of chunk c + 1 are requested BEFORE chunk c is scored (two register sets, the loop unrolled by two): a wave
    // computes ~4 400 VALU cycles per chunk — as long as the HBM round trip — and with two waves per SIMD nothing else would
    // cover that latency (PMC of the first version: waves parked 60 % of their cycles, VALU busy 45 %).
    // MASKED: the bitmap word that holds the chunk's RPC bits travels with its rows — requested here, one chunk ahead of its use, and
    // not looked at before chunk_bits() at scoring time, so the row requests behind it do not wait for it. The chunk is an aligned
    // power-of-two run of rows, so its bits sit inside one word, the same for the whole wave: a scalar load (the bitmap is read
    // through the constant address space — nothing in this kernel writes it) into scalar registers, not vector ones. Per-row
    // attribute values never enter the kernel. Bit i of chunk_bits is row chunk * RPC + i; bits of rows >= n are clear in the bitmap.
    typedef __attribute__((address_space(1))) const f32x4 glb_f32x4;
    auto load_chunk = [&](f32x4 (&v)[MS_U][LOADS], uint32_t (&rr)[MS_U], uint32_t& word, uint32_t chunk) {
        if constexpr (MASKED) {
            typedef __attribute__((address_space(4))) const uint32_t const_u32;
            const uint32_t r0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(chunk * RPC));   // < n: word r0 >> 5 exists
            word = mask != nullptr ? ((const const_u32*)mask)[r0 >> 5] : ~0u;
        }
        const uint32_t rbase = chunk * RPC + sub;
#pragma unroll
        for (int u = 0; u < MS_U; ++u) {
            const uint32_t r = rbase + u * RPW;
            const uint32_t rc = r < n ? r : n - 1;   // clamp: tail lanes re-read the last row, result discarded
            const uint32_t row = LISTED ? rows[rc] : rc;
            rr[u] = row;
            const f32x4* p = store4 + (size_t)row * D4 + gl;
#pragma unroll
            for (int j = 0; j < LOADS; ++j) {
                // MASKED: the rows are read as GLOBAL memory, not through the generic pointer the group table hands over. A skipped
                // chunk's rows are still in flight when the next request names the same registers; for generic (flat) loads, which
                // may complete out of order, the compiler drains every outstanding load first (vmcnt(0) ahead of the prefetch) —
                // global loads return in order and need no such wait.
                if constexpr (MASKED) v[u][j] = __builtin_nontemporal_load((const glb_f32x4*)p + j * GROUP);
                else v[u][j] = __builtin_nontemporal_load(p + j * GROUP);
            }
        }
    };
    auto chunk_bits = [&](uint32_t word, uint32_t chunk) -> uint32_t {
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(chunk * RPC));
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)((word >> (r0 & 31u)) & (uint32_t)((1ull << RPC) - 1ull)));
    };
    auto score_chunk = [&](const f32x4 (&v)[MS_U][LOADS], const uint32_t (&rr)[MS_U], uint32_t bits, uint32_t chunk) {
        const uint32_t rbase = chunk * RPC + sub;
        const uint32_t rr0 = rr[0], rr1 = rr[1], rr2 = rr[2], rr3 = rr[3];   // (named: see row_norm)
        // ||v||^2 per row-group, the norm half of finish_row, then handed to every lane of the group
        // (four named scalars, not an array: a `b4 ? nb[1] : nb[0]` on an array is rewritten into a load from a lane-indexed
        // stack copy — scratch traffic in the hot loop)
        auto row_norm = [&](const f32x4 (&vu)[LOADS]) -> float {
            if (METRIC != M_COS) return 0.f;
            f32x4 nrm = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < LOADS; ++j) accumulate_norm(vu[j], nrm);
            const float tot = group_sum<GROUP>(hsum(nrm));                   // valid in the group's last lane
            return __shfl(tot, last_of_group, 64);
        };
        const float nb0 = row_norm(v[0]), nb1 = row_norm(v[1]), nb2 = row_norm(v[2]), nb3 = row_norm(v[3]);
        static_assert(MS_U == 4, "four row-groups per chunk");
        // lane-private partial sums of all 64 (row-group, query) pairs; query slices come from LDS, one query ahead
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
        // reduce-scatter over the GROUP lanes with group_sum's tree
        ms_halve<0xB1, MS_M>(part, s1);           // quad_perm [1,0,3,2]
        ms_halve<0x4E, MS_M / 2>(part, s2);       // quad_perm [2,3,0,1]
        ms_halve<0x141, MS_M / 4>(part, s3);      // row_half_mirror
        ms_halve<0x140, MS_M / 8>(part, s4);      // row_mirror
        if (GROUP >= 32) ms_halve_rows16<MS_M / 16>(part);
        if (GROUP >= 64) ms_halve_rows32<MS_M / 32>(part);
        // every lane now owns OUT complete sums, all of query q_lane: value index m = j << LEVELS | (selection bits)
#pragma unroll
        for (int j = 0; j < OUT; ++j) {
            int u;
            float nrm;
            uint32_t row;
            if (GROUP == 16) { u = j; nrm = j == 0 ? nb0 : (j == 1 ? nb1 : (j == 2 ? nb2 : nb3)); row = j == 0 ? rr0 : (j == 1 ? rr1 : (j == 2 ? rr2 : rr3)); }
            else if (GROUP == 32) { u = b4 + 2 * j; nrm = j == 0 ? (b4 ? nb1 : nb0) : (b4 ? nb3 : nb2); row = j == 0 ? (b4 ? rr1 : rr0) : (b4 ? rr3 : rr2); }
            else { u = b4 + 2 * b5; nrm = b5 ? (b4 ? nb3 : nb2) : (b4 ? nb1 : nb0); row = b5 ? (b4 ? rr3 : rr2) : (b4 ? rr1 : rr0); }
            const float d = finish_distance<METRIC>(part[j], nrm, qn_lane);
            const uint32_t r = rbase + (uint32_t)u * RPW;
            const int64_t key = make_key(d, row_base + (LISTED ? row : r));
            bool pass = q_live && (r < n) && (key < tau_lane);
            if constexpr (MASKED) pass = pass && ((bits >> (uint32_t)(sub + u * RPW)) & 1u) != 0u;
            unsigned long long todo = __ballot(pass);
            while (todo != 0ull) {                               // rare after warm-up: one list at a time
                const int L = (int)__builtin_ctzll(todo);
                const int qL = __builtin_amdgcn_readlane(q_lane, L);
                const bool same = pass && (q_lane == qL);
                // append inline (a few DS operations); only the prune of a full list runs out of line
                lds_i64* list = (lds_i64*)(my_lists + (size_t)qL * CAP);
                MsState* stq = my_state + qL;
                wave_lds_fence();
                int cnt = __builtin_amdgcn_readfirstlane(stq->cnt);
                const unsigned long long mask = __ballot(same);
                const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                if (same) list[cnt + before] = key;
                cnt += __popcll(mask);
                if (cnt > CAP - 4) {                             // the next push (<= 4 candidates per list) might not fit
                    const PruneOut pr = wave_prune<CAP, true>(list, cnt, k);
                    cnt = pr.cnt;
                    if (q_lane == qL) tau_lane = pr.tau;
                }
                wave_lds_fence();
                if (lane == 0) stq->cnt = cnt;
                todo &= ~mask;
            }
        }
    };
    {
        f32x4 va[MS_U][LOADS], vb[MS_U][LOADS];
        uint32_t ra[MS_U], rb[MS_U];
        uint32_t wa = 0u, wb = 0u;                    // MASKED: the bitmap word of the chunk each set holds (wave-uniform)
        // The prefetch is UNCONDITIONAL (past the end it re-requests the current chunk: L2 hits, discarded): behind a branch
        // the compiler no longer knows how many requests are outstanding and waits vmcnt(0) for the current set — which
        // drains the prefetch it was meant to overlap. MASKED keeps it so: a chunk whose bits are all clear skips its SCORING (a
        // wave-uniform branch around score_chunk), never its loads — which is why a masked group is charged the whole store.
        uint32_t chunk = gwave;
        if (chunk < nchunks) {
            load_chunk(va, ra, wa, chunk);
            for (;;) {
                uint32_t nxt = chunk + nwaves;
                load_chunk(vb, rb, wb, nxt < nchunks ? nxt : chunk);
                __builtin_amdgcn_sched_barrier(0);    // the requests go out before the first use of the current set
                uint32_t bits = MASKED ? chunk_bits(wa, chunk) : 0u;
                if (!MASKED || bits != 0u) score_chunk(va, ra, bits, chunk);
                chunk = nxt;
                if (chunk >= nchunks) break;
                nxt = chunk + nwaves;
                load_chunk(va, ra, wa, nxt < nchunks ? nxt : chunk);
                __builtin_amdgcn_sched_barrier(0);
                bits = MASKED ? chunk_bits(wb, chunk) : 0u;
                if (!MASKED || bits != 0u) score_chunk(vb, rb, bits, chunk);
                chunk = nxt;
                if (chunk >= nchunks) break;
            }
        }
    }

    // per query: sort this wave's list, then rank-merge the workgroup's four lists into the query's partial row
    for (uint32_t qi = 0; qi < nq; ++qi) {
        wave_lds_fence();
        const int cnt = my_state[qi].cnt;
        const PruneOut r = wave_prune<CAP, true>((lds_i64*)(my_lists + (size_t)qi * CAP), cnt, k);
        if (lane == 0) counts[qi * SCAN_WAVES + wave] = r.cnt;
    }
    __syncthreads();
    for (uint32_t qi = 0; qi < nq; ++qi)
        block_rank_merge_impl((const lds_i64*)(lists + (size_t)qi * CAP), SCAN_WAVES, (int)(MS_NQ * CAP),
                              (const lds_i32*)(counts + qi * SCAN_WAVES), k,
                              partial_of(qi));
