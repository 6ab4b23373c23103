// api_batch_masked.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: wax_hip_search_batch_masked — a batch of queries under ONE row predicate, answered by one bf16 MFMA pass over the mirror under
// the predicate's row bitmap and one finish workgroup per query (batch_masked.hip; DESIGN 4.5, "The masked batch pass"). The answer is
// wax_hip_search_batch_predicate's for the same predicate on every query, bit for bit: a query whose certificate fails is re-run in the
// call by the single-query body (search_rows_locked), and everything outside the pass's limits is forwarded to that call unchanged.

int wax_hip_search_batch_masked(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k,
                                const wax_hip_row_predicate* pred, const float* min_scores, uint64_t* out_ids, float* out_scores,
                                uint32_t out_stride, uint32_t* out_counts, uint64_t* stats_out, int32_t grid) {
    // route, queries certified, queries re-run exactly, rows passing the predicate, workgroups, candidates per query, tiles skipped, 0
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto report = [&](int rc) { if (stats_out) std::memcpy(stats_out, stats, sizeof(stats)); return rc; };
    if (!e) return report(fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null"));
    if (nq == 0) return report(WAX_HIP_OK);
    if (!queries || !out_counts || ((!out_ids || !out_scores) && out_stride)) return report(fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null input"));
    if (grid < 0) return report(fail(WAX_HIP_ERR_INVALID_ARGUMENT, "grid must be 0 (default) or a number of row shares"));
    const wax_hip_row_predicate np = normalised_predicate(pred);
    const int kpad = clamp_topk(top_k);
    bool mine = !e->sh && dims == e->dims && batch_masked_dims(dims, e->metric) && kpad <= BM_MAX_K && out_stride > 0 && e->count > 0 &&
                !predicate_is_empty(&np);   // (nothing to test per row: the existing call answers with the unfiltered batch)
    if (mine && nq > kBatchMaxQ) {
        // blocks of kBatchMaxQ queries, one after the other (each its own pass); the words add up, the route is the first block's
        for (uint32_t off = 0; off < nq; off += kBatchMaxQ) {
            uint64_t part[8];
            const uint32_t n = nq - off < kBatchMaxQ ? nq - off : kBatchMaxQ;
            const int rc = wax_hip_search_batch_masked(e, queries + (size_t)off * dims, n, dims, top_k, pred, min_scores ? min_scores + off : nullptr,
                                                       out_ids + (size_t)off * out_stride, out_scores + (size_t)off * out_stride, out_stride,
                                                       out_counts + off, part, grid);
            if (rc != WAX_HIP_OK) return report(rc);
            if (off == 0) std::memcpy(stats, part, sizeof(stats));
            else { stats[1] += part[1]; stats[2] += part[2]; stats[4] += part[4]; stats[6] += part[6]; }
        }
        return report(WAX_HIP_OK);
    }
    if (mine) {
        DeviceGuard g(e->device);
        ReadGuard rd(e);
        { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return report(frc); }
        if (e->row_base + e->count > 0x100000000ull)
            return report(fail(WAX_HIP_ERR_CAPACITY, "row_base + count exceeds UInt32 row indices"));
        const uint32_t n = (uint32_t)e->count;
        const int k = kpad < (int)out_stride ? kpad : (int)out_stride;   // the best out_stride of kpad, as the batched filtered search keeps them
        // a store without attributes reads (0, 0) in every row: the existing call decides such a predicate on the host
        const int entry = (n > 0 && e->cols.has_attributes()) ? pred_entry_acquire(e, np) : -1;
        mine = entry >= 0;                                        // (-1: all four bitmap entries are in use by tickets — forwarded too)
        if (mine) {
            struct EntryUse { wax_hip_engine* e; int idx; ~EntryUse() { pred_entry_release(e, idx); } } use{e, entry};
            BatchCtx* c = nullptr;
            int rc = take_bctx(e, &c);
            if (rc != WAX_HIP_OK) return report(rc);
            hipStream_t st = c->stream;
            BatchMirror& b = e->batch;
            const uint32_t nq_pad = (nq + BM_QUERIES - 1) / BM_QUERIES * BM_QUERIES, qblocks = nq_pad / BM_QUERIES;
            const uint32_t n_tiles = (n + 31u) / 32u;
            uint32_t shares = grid > 0 ? (uint32_t)grid : std::max(1u, resident_cus(e->device) / qblocks);
            if (shares > n_tiles) shares = n_tiles;
            const uint32_t wgs = shares * qblocks;
            // behind the hits in the one download: the certificate words, then the workgroups' skipped tiles
            const uint64_t hit_slots = (uint64_t)nq * k, word_slots = ((uint64_t)nq + wgs + 3) / 4;
            rc = bctx_reserve_host(e, c, nq, hit_slots + word_slots);
            if (rc == WAX_HIP_OK)
                rc = grow_dev(&c->d_rpart, &c->rpart_cap, (uint64_t)nq_pad * shares * (BM_LIST + 2), sizeof(int64_t), "Failed to allocate masked batch lists");
            if (rc == WAX_HIP_OK) rc = ensure_mirror(e, st);
            const uint32_t* d_bitmap = nullptr;
            if (rc == WAX_HIP_OK) rc = pred_entry_prepare(e, entry, st, &d_bitmap);
            if (rc == WAX_HIP_OK && (b.d_cb == nullptr || b.d_maxnorm == nullptr)) rc = fail(WAX_HIP_ERR_INTERNAL, "the bf16 mirror is not there");
            uint32_t* d_cert = reinterpret_cast<uint32_t*>(c->d_hits + hit_slots);
            const uint32_t* h_cert = reinterpret_cast<const uint32_t*>(c->h_hits + hit_slots);
            hipError_t err = hipSuccess;
            if (rc == WAX_HIP_OK) {
                err = hipMemcpyAsync(c->d_q, queries, (size_t)nq * dims * sizeof(float), hipMemcpyHostToDevice, st);
                // the queries as bf16 fragments, their exact norms, and eps from the mirror's measured error norms (batch_prep_kernel)
                PrepArgs pa{};
                pa.queries = c->d_q; pa.nq = nq; pa.nq_pad = nq_pad; pa.dims = dims; pa.metric = e->metric;
                pa.max_bits = b.d_maxnorm; pa.use_measured = e->batch_eps_measured.load() != 0 ? 1 : 0;
                pa.qb = c->d_qb; pa.qf = c->d_qf; pa.q_n2 = c->d_qn2; pa.q_norm = c->d_qnorm; pa.eps = c->d_eps; pa.tau = c->d_tau; pa.overflow = c->d_overflow;
                if (err == hipSuccess) err = launch_batch_prep(pa, st);
                BatchMaskedArgs a{};
                a.mirror = b.d_cb; a.qf = c->d_qf; a.bitmap = d_bitmap; a.lists = c->d_rpart; a.bounds = c->d_rpart + (size_t)nq_pad * shares * BM_LIST;
                a.skipped = d_cert + nq; a.n_rows = n; a.row_base = (uint32_t)e->row_base; a.dims = dims; a.nq_pad = nq_pad; a.shares = shares;
                if (err == hipSuccess) err = launch_batch_masked(a, e->metric, st);
                BatchMaskedFinishArgs f{};
                f.lists = a.lists; f.bounds = a.bounds; f.store = e->d_store; f.queries = c->d_q; f.q_norm = c->d_qnorm; f.eps = c->d_eps; f.ids = e->d_ids;
                f.hits = c->d_hits; f.certified = d_cert; f.n_rows = n; f.row_base = a.row_base; f.dims = dims; f.nq = nq; f.shares = shares; f.k = k;
                if (err == hipSuccess) err = launch_batch_masked_finish(f, e->metric, st);
                if (err == hipSuccess) err = hipMemcpyAsync(c->h_hits, c->d_hits, (size_t)(hit_slots + word_slots) * sizeof(wax_hip_hit), hipMemcpyDeviceToHost, st);
                if (err == hipSuccess) err = hipStreamSynchronize(st);
                if (err != hipSuccess) rc = fail(WAX_HIP_ERR_INTERNAL, std::string("masked batch failed on device: ") + hipGetErrorString(err));
            }
            if (rc != WAX_HIP_OK) (void)hipStreamSynchronize(st);
            std::vector<uint32_t> rerun;
            if (rc == WAX_HIP_OK) {
                for (uint32_t q = 0; q < nq; ++q) {
                    if (h_cert[q] == 0u) { rerun.push_back(q); continue; }
                    uint32_t m = 0;
                    hits_to_results(e->metric, c->h_hits + (size_t)q * k, (uint32_t)k, out_ids + (size_t)q * out_stride, out_scores + (size_t)q * out_stride, out_stride, &m);
                    if (min_scores) apply_min_score(min_scores[q], out_ids + (size_t)q * out_stride, out_scores + (size_t)q * out_stride, &m);
                    out_counts[q] = m;
                }
                for (uint32_t s = 0; s < shares; ++s) stats[6] += h_cert[nq + s];   // (every query block skips the same tiles: the first one's)
                uint64_t passing = 0, tiles = 0;
                if (pred_entry_counts(e, entry, true, &passing, &tiles)) stats[3] = passing;
                e->st_rows += (uint64_t)(n_tiles - stats[6]) * 32u * qblocks;
                e->st_bytes += (uint64_t)(n_tiles - stats[6]) * 32u * qblocks * dims * 2ull + (uint64_t)nq * BM_CAND * dims * 4ull;
            }
            e->bctxs.release(c);
            // the uncertified queries: the exact route of one filtered query, under the lock this call already holds
            for (size_t i = 0; rc == WAX_HIP_OK && i < rerun.size(); ++i) {
                const uint32_t q = rerun[i];
                uint32_t m = 0;
                rc = search_rows_locked(e, queries + (size_t)q * dims, dims, kpad, 0, nullptr, 0, &np,
                                        out_ids + (size_t)q * out_stride, out_scores + (size_t)q * out_stride, out_stride, &m, nullptr);
                if (rc != WAX_HIP_OK) break;
                if (min_scores) apply_min_score(min_scores[q], out_ids + (size_t)q * out_stride, out_scores + (size_t)q * out_stride, &m);
                out_counts[q] = m;
            }
            if (rc == WAX_HIP_OK) {
                stats[0] = 1; stats[1] = nq - rerun.size(); stats[2] = rerun.size(); stats[4] = wgs;
                stats[5] = std::min<uint64_t>((uint64_t)shares * BM_LIST, (uint64_t)BM_CAND);
            }
            return report(rc);
        }
    }
    // a sharded handle, L2, a dimension outside {384, 768}, k > 32, an empty store, a store without attributes, an empty predicate, no free bitmap entry: route 0
    std::vector<wax_hip_row_predicate> preds(pred ? nq : 0, np);
    return report(wax_hip_search_batch_predicate(e, queries, nq, dims, top_k, nullptr, 0, nullptr, nullptr, min_scores, pred ? preds.data() : nullptr,
                                                 out_ids, out_scores, out_stride, out_counts));
}
