// api_batch_resident.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: wax_hip_search_batch_resident — wax_hip_search_batch_hits' answer, bit for bit, for a store that sits in L2 / MALL: every
// (row, query) pair scored exactly in f32 and selected in ONE launch per block of up to 1 024 queries (batch_resident.hip; DESIGN 4.4,
// "The resident batch"). No mirror, no certificate, no retry; anything outside its limits is handed to search_batch_hits unchanged.

// Largest store the call answers itself. Measured with the limit at 16 384 (profiles/r36/batch_resident.json, blocking call, 256 queries,
// top-10, medians of 15): the call is BEHIND search_batch_hits at every size — 384-d 137 / 173 / 254 / 386 us against 99 / 134 / 117 / 106
// at 1 000 / 3 000 / 8 192 / 16 384 rows — so there is no crossover above 4 096 rows and the limit is 4 096: what remains are the stores
// search_batch_hits serves by shared exact passes or the per-query loop (top-100 on 3 000 rows x 256 queries: 477 us against 1 975).
constexpr uint64_t RESIDENT_MAX_ROWS = 4096;

static uint32_t resident_cus(int device) {   // compute units of the device (asked once per device)
    static std::atomic<uint32_t> cached[64] = {};
    const int slot = device & 63;
    uint32_t n = cached[slot].load(std::memory_order_relaxed);
    if (n == 0) {
        int v = 0;
        n = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && v > 0) ? (uint32_t)v : 256u;
        cached[slot].store(n, std::memory_order_relaxed);
    }
    return n;
}

int wax_hip_search_batch_resident(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k,
                                  wax_hip_hit* out_hits, uint32_t out_stride, uint32_t* out_counts, uint64_t* stats_out) {
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // route, launches, query blocks per launch, row shares, tile rows, queries per block, 0, 0
    auto report = [&](int rc) { if (stats_out) std::memcpy(stats_out, stats, sizeof(stats)); return rc; };
    if (!e) return report(fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null"));
    if (nq == 0) return report(WAX_HIP_OK);
    if (!queries || !out_counts || (!out_hits && out_stride)) return report(fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null input"));
    const uint64_t limit = (uint64_t)clamp_topk(top_k);
    // (the row count is a first look; the lock below decides)
    bool mine = !e->sh && out_stride > 0 && dims == e->dims && batch_resident_dims(dims) && limit <= (uint64_t)FUSED_MAX_K &&
                e->count > 0 && e->count <= RESIDENT_MAX_ROWS && e->force_general.load() == 0;
    int rc = WAX_HIP_OK;
    if (mine) {
        DeviceGuard g(e->device);
        ReadGuard rd(e);
        { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return report(frc); }
        if (e->row_base + e->count > 0x100000000ull)
            return report(fail(WAX_HIP_ERR_CAPACITY, "row_base + count exceeds UInt32 row indices"));
        const uint64_t n = e->count;                          // the row count this batch is answered on
        uint64_t k64 = limit < n ? limit : n;
        if (k64 > out_stride) k64 = out_stride;               // a smaller result array: the best `stride` of them
        mine = n > 0 && n <= RESIDENT_MAX_ROWS && k64 > 0;
        if (mine) {
            const int k_eff = (int)k64;
            const uint32_t per_launch = nq < RESIDENT_MAX_Q ? nq : RESIDENT_MAX_Q;
            const uint32_t blocks = (per_launch + 15u) / 16u;
            const uint32_t shares = batch_resident_shares(blocks, k_eff, resident_cus(e->device));
            BatchCtx* c = nullptr;
            rc = take_bctx(e, &c);
            if (rc != WAX_HIP_OK) return report(rc);
            hipStream_t st = c->stream;
            // the norms ride behind the queries in the staging block: [nq][dims] floats, then [nq]
            std::vector<float> norms(nq);
            for (uint32_t q = 0; q < nq; ++q) norms[q] = query_norm(queries + (size_t)q * dims, dims);
            rc = bctx_reserve_host(e, c, (uint64_t)nq + ((uint64_t)nq + dims - 1) / dims, (uint64_t)nq * k_eff);
            if (rc == WAX_HIP_OK)
                rc = grow_dev(&c->d_rpart, &c->rpart_cap, (uint64_t)blocks * 16u * shares * (uint64_t)k_eff, sizeof(int64_t), "Failed to allocate resident partial lists");
            hipError_t err = hipSuccess;
            if (rc == WAX_HIP_OK && !c->d_rarrive) {
                // zeroed once, by a memset that precedes the first launch on this stream; every launch leaves them at zero
                err = hipMalloc(reinterpret_cast<void**>(&c->d_rarrive), (RESIDENT_MAX_Q / 16u) * sizeof(uint32_t));
                if (err == hipSuccess) err = hipMemsetAsync(c->d_rarrive, 0, (RESIDENT_MAX_Q / 16u) * sizeof(uint32_t), st);
                if (err != hipSuccess) { (void)hipFree(c->d_rarrive); c->d_rarrive = nullptr; rc = fail(WAX_HIP_ERR_ALLOC, std::string("Failed to allocate resident arrival counters: ") + hipGetErrorString(err)); }
            }
            float* d_norm = c->d_q + (size_t)nq * dims;
            bool launched = false;
            if (rc == WAX_HIP_OK) {
                err = hipMemcpyAsync(c->d_q, queries, (size_t)nq * dims * sizeof(float), hipMemcpyHostToDevice, st);
                if (err == hipSuccess) err = hipMemcpyAsync(d_norm, norms.data(), (size_t)nq * sizeof(float), hipMemcpyHostToDevice, st);
                if (err != hipSuccess) rc = fail(WAX_HIP_ERR_INTERNAL, std::string("query upload: ") + hipGetErrorString(err));
            }
            uint32_t launches = 0;
            for (uint32_t off = 0; rc == WAX_HIP_OK && off < nq; off += RESIDENT_MAX_Q) {   // consecutive launches, one stream, one workspace
                ResidentArgs a{};
                a.store = e->d_store; a.queries = c->d_q + (size_t)off * dims; a.q_norm = d_norm + off; a.ids = e->d_ids;
                a.partials = c->d_rpart; a.arrive = c->d_rarrive; a.out = c->d_hits + (size_t)off * k_eff;
                a.n_rows = (uint32_t)n; a.row_base = (uint32_t)e->row_base; a.nq = nq - off < RESIDENT_MAX_Q ? nq - off : RESIDENT_MAX_Q;
                a.k = (uint32_t)k_eff; a.out_stride = (uint32_t)k_eff;
                err = launch_batch_resident(a, dims, e->metric, shares, st);
                if (err != hipSuccess) rc = fail(WAX_HIP_ERR_INTERNAL, std::string("resident batch launch: ") + hipGetErrorString(err));
                launched = true;
                ++launches;
            }
            if (rc == WAX_HIP_OK) {
                err = hipMemcpyAsync(c->h_hits, c->d_hits, (size_t)nq * k_eff * sizeof(wax_hip_hit), hipMemcpyDeviceToHost, st);
                if (err == hipSuccess) err = hipStreamSynchronize(st);
                if (err != hipSuccess) rc = fail(WAX_HIP_ERR_INTERNAL, std::string("resident batch failed on device: ") + hipGetErrorString(err));
            }
            if (rc == WAX_HIP_OK) {
                for (uint32_t q = 0; q < nq; ++q) {
                    wax_hip_hit* row = out_hits + (size_t)q * out_stride;
                    std::memcpy(row, c->h_hits + (size_t)q * k_eff, (size_t)k_eff * sizeof(wax_hip_hit));
                    uint32_t m = 0;
                    for (int i = 0; i < k_eff; ++i) m += row[i].key != KEY_PAD;
                    for (uint32_t i = (uint32_t)k_eff; i < out_stride; ++i) row[i] = wax_hip_hit{KEY_PAD, ID_PAD};
                    out_counts[q] = m;
                }
                stats[0] = 1; stats[1] = launches; stats[2] = blocks; stats[3] = shares;
                stats[4] = batch_resident_tile_rows(dims); stats[5] = 16;
            } else {
                (void)hipStreamSynchronize(st);
                // a launch that did not run to its end may have left tickets behind: the next call's launch finds zeros again
                if (launched && c->d_rarrive) { (void)hipMemsetAsync(c->d_rarrive, 0, (RESIDENT_MAX_Q / 16u) * sizeof(uint32_t), st); (void)hipStreamSynchronize(st); }
            }
            e->bctxs.release(c);
            return report(rc);
        }
    }
    // a sharded handle, a dimension outside the table, k > 192, a store above RESIDENT_MAX_ROWS (or empty), "force_general": route 0
    return report(wax_hip_search_batch_hits(e, queries, nq, dims, top_k, out_hits, out_stride, out_counts));
}
