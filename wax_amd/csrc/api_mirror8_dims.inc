// api_mirror8_dims.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: wax_hip_search_mirror_codes — wax_hip_search_mirror's call (api_mirror_dims.inc) answered from the 8-bit code mirror: up to
// 1 024 queries of a cosine or dot store at 512, 1 024 or 1 536 dimensions, optionally under ONE row predicate, in ceil(nq / 4) passes
// of up to four queries on the int8 matrix pipe (mirror8_dims.hip; DESIGN 4.1, "The code mirror at 512, 1 024 and 1 536 dimensions"),
// each behind its selection, re-score and finish, all on one stream in front of one synchronisation. Row q of the answer is
// wax_hip_search's (wax_hip_search_predicate's under a predicate) for query q, bit for bit: a query whose certificate fails is re-run
// in the call on the route that answers it today, and everything outside the pass's limits is forwarded to that call unchanged.

int wax_hip_search_mirror_codes(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, uint32_t top_k,
                                const wax_hip_row_predicate* pred, uint64_t* ids_out, float* scores_out, uint32_t* counts_out,
                                uint64_t* stats_out) {
    // route, passes, queries certified, queries re-run, lists per pass, tiles skipped, candidates per query, 0
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto report = [&](int rc) { if (stats_out) std::memcpy(stats_out, stats, sizeof(stats)); return rc; };
    if (!e) return report(fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null"));
    if (nq == 0) return report(WAX_HIP_OK);
    if (!queries || !ids_out || !scores_out || !counts_out) return report(fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null input"));
    if (nq > kBatchMaxQ) return report(fail(WAX_HIP_ERR_INVALID_ARGUMENT, "searchMirror: at most 1024 queries per call"));
    const int32_t tk = top_k > 0x7fffffffu ? 0x7fffffff : (int32_t)top_k;
    const int kpad = clamp_topk(tk);
    const uint32_t stride = (uint32_t)kpad;                      // entries per row of ids_out / scores_out: wax_hip_result_capacity(top_k)
    const wax_hip_row_predicate np = normalised_predicate(pred);
    const bool has_pred = !predicate_is_empty(&np);
    bool mine = !e->sh && dims == e->dims && mirror8_dims_supported(dims, (int)e->metric) && kpad <= MIRROR8_MAX_K && e->count > 0;
    if (mine) {
        DeviceGuard g(e->device);
        ReadGuard rd(e);
        { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return report(frc); }
        if (e->row_base + e->count > 0x100000000ull)
            return report(fail(WAX_HIP_ERR_CAPACITY, "row_base + count exceeds UInt32 row indices"));
        const uint32_t n = (uint32_t)e->count;
        // a store without attributes reads (0, 0) in every row: the existing call decides such a predicate on the host
        const int entry = (n > 0 && has_pred && e->cols.has_attributes()) ? pred_entry_acquire(e, np) : -1;
        mine = n > 0 && (!has_pred || entry >= 0);                // (-1 under a predicate: no attributes, or all four bitmap entries are in use by tickets)
        if (mine) {
            struct EntryUse { wax_hip_engine* e; int idx; ~EntryUse() { pred_entry_release(e, idx); } } use{e, entry};
            BatchCtx* c = nullptr;
            int rc = take_bctx(e, &c);
            if (rc != WAX_HIP_OK) return report(rc);
            hipStream_t st = c->stream;
            BatchMirror& b = e->batch;
            const int k = (uint32_t)kpad < n ? kpad : (int)n;
            const int grid_cap = (int)e->grid_blocks.load();
            const int lists = mirror8_dims_grid(n, dims, grid_cap);
            const uint32_t passes = (nq + MIRROR_MAX_NQ - 1) / MIRROR_MAX_NQ;
            // behind the hits in the one download: the certificate words
            const uint64_t hit_slots = (uint64_t)nq * k, word_slots = ((uint64_t)nq + 3) / 4;
            rc = bctx_reserve_host(e, c, nq, hit_slots + word_slots);
            // four sets of lists, candidates, exact keys and control words, reused from pass to pass: the stream orders a pass behind
            // the finish that read them
            const uint64_t list_words = (uint64_t)MIRROR_MAX_NQ * lists * MIRROR_KP, cand_words = (uint64_t)MIRROR_MAX_NQ * MIRROR8_DIMS_C;
            if (rc == WAX_HIP_OK)
                rc = grow_dev(&c->d_rpart, &c->rpart_cap, list_words + 2 * cand_words + (uint64_t)MIRROR_MAX_NQ * MIRROR_WIDE_CTL, sizeof(int64_t),
                              "Failed to allocate code mirror pass lists");
            if (rc == WAX_HIP_OK) rc = ensure_mirror8(e, st);
            const uint32_t* d_bitmap = nullptr;
            if (rc == WAX_HIP_OK && has_pred) rc = pred_entry_prepare(e, entry, st, &d_bitmap);
            if (rc == WAX_HIP_OK && (b.d_c8 == nullptr || b.d_c8_meta == nullptr || b.d_c8_max == nullptr)) rc = fail(WAX_HIP_ERR_INTERNAL, "the code mirror is not there");
            uint32_t* d_cert = reinterpret_cast<uint32_t*>(c->d_hits + hit_slots);
            const uint32_t* h_cert = reinterpret_cast<const uint32_t*>(c->h_hits + hit_slots);
            if (rc == WAX_HIP_OK) {
                hipError_t err = hipMemcpyAsync(c->d_q, queries, (size_t)nq * dims * sizeof(float), hipMemcpyHostToDevice, st);
                Mirror8DimsArgs a{};
                a.ga.codes = b.d_c8; a.ga.meta = b.d_c8_meta;
                a.cand = c->d_rpart + list_words; a.exact = a.cand + cand_words; a.ctl = reinterpret_cast<uint64_t*>(a.exact + cand_words);
                MirrorScanArgs& s = a.ga.g.a;
                s.store = e->d_store; s.ids = e->d_ids; s.max_bits = b.d_c8_max;
                s.n_rows = n; s.row_base = (uint32_t)e->row_base; s.dims = dims;
                for (uint32_t q0 = 0; err == hipSuccess && q0 < nq; q0 += MIRROR_MAX_NQ) {
                    const int members = (int)(nq - q0 < (uint32_t)MIRROR_MAX_NQ ? nq - q0 : (uint32_t)MIRROR_MAX_NQ);
                    for (int i = 0; i < members; ++i) {
                        MirrorMember& m = a.ga.g.m[i];
                        m.query = c->d_q + (size_t)(q0 + i) * dims;
                        m.partials = c->d_rpart + (size_t)i * lists * MIRROR_KP;
                        m.hits = c->d_hits + (size_t)(q0 + i) * k;
                        m.certified = d_cert + q0 + i;
                        m.bitmap = d_bitmap;
                        m.q_norm = query_norm(queries + (size_t)(q0 + i) * dims, dims);
                        m.k = k; m.kpad = k;
                    }
                    err = launch_mirror8_dims(a, members, (int)e->metric, grid_cap, st);
                }
                if (err == hipSuccess) err = hipMemcpyAsync(c->h_hits, c->d_hits, (size_t)(hit_slots + word_slots) * sizeof(wax_hip_hit), hipMemcpyDeviceToHost, st);
                if (err == hipSuccess) err = hipStreamSynchronize(st);
                if (err != hipSuccess) rc = fail(WAX_HIP_ERR_INTERNAL, std::string("code mirror search failed on device: ") + hipGetErrorString(err));
            }
            if (rc != WAX_HIP_OK) (void)hipStreamSynchronize(st);
            std::vector<uint32_t> rerun;
            if (rc == WAX_HIP_OK) {
                for (uint32_t q = 0; q < nq; ++q) {
                    if (h_cert[q] == 0u) { rerun.push_back(q); continue; }
                    uint32_t m = 0;
                    hits_to_results(e->metric, c->h_hits + (size_t)q * k, (uint32_t)k, ids_out + (size_t)q * stride, scores_out + (size_t)q * stride, stride, &m);
                    counts_out[q] = m;
                }
                // what the passes read: every 16-row tile, or under a bitmap the tiles that hold a passing row — the pass's own unit,
                // counted when the bitmap was built
                const uint64_t tiles = ((uint64_t)n + 15) / 16;
                uint64_t rows_read = (uint64_t)n, passing = 0, live_tiles = 0;
                if (has_pred && pred_entry_counts(e, entry, true, &passing, &live_tiles) && live_tiles <= tiles) {
                    stats[5] = (tiles - live_tiles) * passes;
                    rows_read = live_tiles * 16ull;
                }
                e->st_rows += rows_read * passes;
                e->st_bytes += rows_read * passes * ((uint64_t)dims + 8ull) + (uint64_t)nq * MIRROR8_DIMS_C * dims * 4ull;
            }
            e->bctxs.release(c);
            // the uncertified queries (ties, duplicate rows, a clustered store, a NaN query), under the lock this call already holds:
            // the f32 scan, or under a predicate the exact route of one filtered query
            for (size_t i = 0; rc == WAX_HIP_OK && i < rerun.size(); ++i) {
                const uint32_t q = rerun[i];
                const float* query = queries + (size_t)q * dims;
                uint32_t m = 0;
                if (has_pred) {
                    rc = search_rows_locked(e, query, dims, kpad, 0, nullptr, 0, &np, ids_out + (size_t)q * stride, scores_out + (size_t)q * stride, stride, &m, nullptr);
                } else {
                    uint64_t t = 0;
                    rc = submit_impl(e, query, dims, tk, &t, false, /*caller_locked=*/true);
                    if (rc == WAX_HIP_OK)
                        rc = collect_impl(e, t, ids_out + (size_t)q * stride, scores_out + (size_t)q * stride, stride, &m, nullptr, 0, /*caller_locked=*/true);
                }
                counts_out[q] = m;
            }
            if (rc == WAX_HIP_OK) {
                stats[0] = 1; stats[1] = passes; stats[2] = nq - rerun.size(); stats[3] = rerun.size(); stats[4] = (uint64_t)lists;
                stats[6] = (uint64_t)MIRROR8_DIMS_C;
            }
            return report(rc);
        }
    }
    // a sharded handle, L2, every other dimension (384 and 768 keep their own routes), k > 16, an empty store, a predicate on a store
    // without attributes, no free bitmap entry: route 0 — the existing search, query by query
    for (uint32_t q = 0; q < nq; ++q) {
        const float* query = queries + (size_t)q * dims;
        const int rc = has_pred ? wax_hip_search_predicate(e, query, dims, tk, 0, nullptr, 0, 0, 0.f, &np, ids_out + (size_t)q * stride,
                                                           scores_out + (size_t)q * stride, stride, counts_out + q)
                                : wax_hip_search(e, query, dims, tk, ids_out + (size_t)q * stride, scores_out + (size_t)q * stride, stride, counts_out + q);
        if (rc != WAX_HIP_OK) return report(rc);
    }
    return report(WAX_HIP_OK);
}
