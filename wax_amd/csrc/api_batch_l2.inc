// api_batch_l2.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: wax_hip_search_batch_l2 — wax_hip_search_batch_hits' answer, bit for bit, for L2 stores at 384 and 768 dimensions, with the
// one-pass pipeline's filtering launch on the register-resident L2 GEMM (batch_rq_l2.hip; DESIGN 4.4, "The register-resident L2
// filter"). Sampling, thresholds, the counted candidate list, the finish and the exact ladder are search_batch_hits' own
// (batch_hits_mfma, api_batch.inc); anything else is handed to wax_hip_search_batch_hits unchanged.

int wax_hip_search_batch_l2(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k,
                            wax_hip_hit* out_hits, uint32_t out_stride, uint32_t* out_counts, uint64_t* stats_out) {
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // route, queries, queries answered by the exact ladder, workgroups, rows per tile, queries per workgroup, 0, 0
    auto report = [&](int rc) { if (stats_out) std::memcpy(stats_out, stats, sizeof(stats)); return rc; };
    if (!e) return report(fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null"));
    if (nq == 0) return report(WAX_HIP_OK);
    if (!queries || !out_counts || (!out_hits && out_stride)) return report(fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null input"));
    // (a first look; batch_hits_mfma decides under the lock, with the planner)
    const bool mine = !e->sh && out_stride > 0 && dims == e->dims && batch_rq_l2_dims(dims, (int)e->metric) && e->count > 0 &&
                      e->force_general.load() == 0;
    if (mine) {
        for (uint32_t q = 0; q < nq; ++q) out_counts[q] = 0;
        for (size_t i = 0; i < (size_t)nq * out_stride; ++i) out_hits[i] = wax_hip_hit{KEY_PAD, ID_PAD};
        KsplitReport ks;
        ks.kernel = BATCH_FILTER_RQ_L2;
        bool ran = false;
        const int rc = batch_hits_mfma(e, queries, nq, dims, (uint64_t)clamp_topk(top_k), out_hits, out_stride, out_counts, &ks, &ran);
        if (rc != WAX_HIP_OK) return report(rc);
        if (ran) {
            stats[0] = 1; stats[1] = nq; stats[2] = ks.fallbacks; stats[3] = ks.workgroups; stats[4] = ks.tile_rows; stats[5] = BATCH_GROUP_QUERIES;
            return report(WAX_HIP_OK);
        }
    }
    // a sharded handle, cosine / dot, another dimension, a store the one-pass planner does not take, "force_general": route 0
    return report(wax_hip_search_batch_hits(e, queries, nq, dims, top_k, out_hits, out_stride, out_counts));
}
