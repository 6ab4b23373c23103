// tuning.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: stats, the tuning registry (set / get), the two timing microbenchmarks

// ---- observability / tuning -----------------------------------------------

int wax_hip_stats(wax_hip_engine* e, wax_hip_stats_t* out) {
    if (!e || !out) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (e->sh) return sh_stats(e, out);
    out->searches = e->st_searches.load();
    out->rows_scanned = e->st_rows.load();
    out->bytes_scanned = e->st_bytes.load();
    out->transient_allocations = e->st_alloc.load();
    out->reuse_count = e->st_reuse.load();
    out->reserved_rows = e->capacity;
    {
        DeviceGuard g(e->device);
        for (int r = 0; r < kShardRing; ++r) harvest_ring_event(e, r);
    }
    std::unique_lock<std::mutex> sg(e->st_mu);
    out->last_scan_kernel_ms = e->st_last_ms;
    out->scan_kernel_ms_total = e->st_total_ms;
    out->scan_kernels_timed = e->st_timed;
    out->batch_gemm_ms_total = e->st_gemm_ms;
    out->batch_gemms_timed = e->st_gemm_timed;
    out->batch_gemm_rows = e->st_gemm_rows;
    out->batch_gemm_queries = e->st_gemm_queries;
    return WAX_HIP_OK;
}

int wax_hip_set_tuning(wax_hip_engine* e, const char* key, int64_t value) {
    if (!e || !key) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    const std::string k(key);
    if (e->sh) return sh_set_tuning(e, k, value);
    if (k == "grid_blocks") e->grid_blocks = value;
    else if (k == "variant") e->variant = value;
    else if (k == "time_kernels") e->time_kernels = value;
    else if (k == "force_general") e->force_general = value;
    else if (k == "select_grid") { if (value < 0 || value > 2048) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "select_grid must be 0 (auto) .. 2048"); e->select_grid = value; }
    else if (k == "select_short") { if (value < 0 || value > 2) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "select_short must be 0, 1 or 2"); e->select_short = value; }
    else if (k == "stream_nt") e->stream_nt = value;
    else if (k == "fuse_merge") e->fuse_merge = value != 0;
    else if (k == "done_flag") e->done_flag = value != 0;
    else if (k == "merge_kway") e->merge_kway = value != 0;
    else if (k == "merge_overlap_mb") e->merge_overlap_mb = value < 0 ? 0 : value;
    else if (k == "batch_qfrag") e->batch_qfrag = value != 0;
    else if (k == "scan_plain_mb") e->scan_plain_mb = value;
    else if (k == "scan_mirror") { if (value < 0 || value > 2) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "scan_mirror must be 0, 1 or 2"); e->scan_mirror = value; }
    else if (k == "mirror_share") { if (value < 0 || value > 2) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror_share must be 0, 1 or 2"); e->mirror_share = value; }
    else if (k == "mirror_bits") { if (value != 0 && value != 8 && value != 16) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror_bits must be 0, 8 or 16"); e->mirror_bits = value; }
    else if (k == "mirror_fill") { if (value < 0 || value > 1) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror_fill must be 0 or 1"); e->mirror_fill = value; }
    else if (k == "query_args") { if (value < 0 || value > 2) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "query_args must be 0, 1 or 2"); e->query_args = value; }
    else if (k == "batch_min") e->batch_min = value;
    else if (k == "batch_mode") e->batch_mode = value;
    else if (k == "batch_rega") { if (value != 0 && value != 1 && value != 5) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "batch_rega must be 0, 1 or 5"); e->batch_rega = value; }
    else if (k == "batch_dyn_tail") { if (value != 0 && value != 1) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "batch_dyn_tail must be 0 or 1"); e->batch_dyn_tail = value; }
    else if (k == "batch_host_multi") { if (value != 0 && value != 1) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "batch_host_multi must be 0 or 1"); e->batch_host_multi = value; }
    else if (k == "batch_in_wait") { if (value != 0 && value != 1) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "batch_in_wait must be 0 or 1"); e->batch_in_wait = value; }
    else if (k == "batch_debug") { if (value & ~(int64_t)(4096 | 16384 | 65536)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "batch_debug: bits 4096, 16384, 65536 only"); e->batch_debug = value; }
    else if (k == "batch_prof_ptr") e->batch_prof_ptr = value;
    else if (k == "batch_onepass") e->batch_onepass = value;
    else if (k == "batch_onepass_tiles") { if (value < 32) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "batch_onepass_tiles must be >= 32"); e->batch_onepass_tiles = value; }
    else if (k == "batch_kp_fused") e->batch_kp_fused = value != 0;
    else if (k == "batch_survivors") { if (value < 2 || value > 64) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "batch_survivors must be 2..64"); e->batch_survivors = value; }
    else if (k == "batch_eps_measured") e->batch_eps_measured = value != 0;
    else if (k == "retry_hint") {   // > 0: the next `value` clean batches still carry the device-side retry kernel (set by collect; tests force it)
        if (value < 0 || value > 1024) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "retry_hint must be 0..1024");
        e->retry_hint = (int)value;
    }
    else if (k == "batch_retry") { if (value < 0 || value > 2) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "batch_retry must be 0, 1 or 2"); e->batch_retry = value; }
    else if (k == "batch_multi") e->batch_multi = value != 0;
    else if (k == "scan_chain") { if (value < -1 || value > 1) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "scan_chain must be -1 (auto), 0 or 1"); e->scan_chain = value; }
    else if (k == "share_timing") e->share_timing = value != 0;   // 0: every chained scan records its own start event (one more packet between scans)
    else if (k == "filter_batch") { if (value < 0 || value > 1) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "filter_batch must be 0 or 1"); e->filter_batch = value; }
    else if (k == "predicate_batch_rows") { if (value < 0 || value > 0x7fffffffll) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "predicate_batch_rows must be 0..2147483647"); e->predicate_batch_rows = value; }
    else if (k == "filter_device_min") { if (value < -1) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "filter_device_min must be >= -1"); e->filter_device_min = value; }
    else if (k == "search_many") { if (value < 0 || value > 1) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "search_many must be 0 or 1"); e->search_many = value; }
    else if (k == "search_many_max_rows") { if (value < 0 || value > 0xffffffffll) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "search_many_max_rows must be 0..4294967295"); e->search_many_max_rows = value; }
    else if (k == "predicate_route") { if (value < 0 || value > 2) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "predicate_route must be 0 (auto), 1 (gather) or 2 (masked scan)"); e->predicate_route = value; }
    else if (k == "predicate_mirror") { if (value < 0 || value > 2) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "predicate_mirror must be 0 (never), 1 (auto) or 2 (every store)"); e->predicate_mirror = value; }
    else if (k == "predicate_scan_min_permille") { if (value < 0 || value > 1001) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "predicate_scan_min_permille must be 0..1001"); e->predicate_scan_min_permille = value; }
    else if (k == "compact_window_rows") { if (value < 0 || value > 0xffffffffll) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "compact_window_rows must be 0 (what the bounce buffer holds) .. 4294967295"); e->compact_window_rows = value; }
    else if (k == "batch_sample_div") { if (value < 4 || value > 4096) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "batch_sample_div must be 4..4096"); e->batch_sample_div = value; }
    else if (k == "batch_workspaces") {
        if (value < 1 || value > 16) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "batch_workspaces must be 1..16");
        std::unique_lock<std::mutex> g(e->bctx_mu);
        e->bctx_max = (int)value;
    }
    else if (k == "batch_first") { if (value < 128 || value > kBatchFirstSlab || value % 128) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "batch_first must be a multiple of 128 in 128..2048"); e->batch_first = value; }
    else if (k == "batch_growth") { if (value < 1 || value > 64) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "batch_growth must be 1..64"); e->batch_growth = value; }
    else if (k == "batch_slab_mb") { if (value < 1 || value > 4096) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "batch_slab_mb must be 1..4096"); e->batch_slab_mb = value; }
    else if (k == "streams") {
        if (value < 1 || value > kMaxStreams) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "streams must be 1..4");
        std::unique_lock<std::mutex> g(e->slot_mu);
        e->n_streams = (int)value;
    } else if (k == "slots") {
        if (value < 1 || value > 64) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "slots must be 1..64");
        std::unique_lock<std::mutex> g(e->slot_mu);
        e->max_slots = (int)value;
    } else if (k == "reset_stats") {
        e->st_searches = 0; e->st_rows = 0; e->st_bytes = 0;
        {
            DeviceGuard g(e->device);
            for (int r = 0; r < kShardRing; ++r) harvest_ring_event(e, r);
        }
        std::unique_lock<std::mutex> sg(e->st_mu);
        e->st_last_ms = 0; e->st_total_ms = 0; e->st_timed = 0;
        e->st_gemm_ms = 0; e->st_gemm_timed = 0; e->st_gemm_rows = 0; e->st_gemm_queries = 0;
    } else return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "unknown tuning key '" + k + "'");
    return WAX_HIP_OK;
}

int64_t wax_hip_get_tuning(wax_hip_engine* e, const char* key) {
    if (!e || !key) return -1;
    const std::string k(key);
    if (e->sh) return sh_get_tuning(e, k);
    if (k == "grid_blocks") return e->grid_blocks.load();
    if (k == "variant") return e->variant.load();
    if (k == "time_kernels") return e->time_kernels.load();
    if (k == "force_general") return e->force_general.load();
    if (k == "select_short") return e->select_short.load();
    if (k == "select_grid") return e->select_grid.load();
    if (k == "short_selects") return (int64_t)e->st_short_selects.load();
    if (k == "short_select_failures") {   // short selections whose certificate failed (the long path answered): device words of every slot; a blocking read
        int64_t t = 0;
        DeviceGuard g(e->device);
        (void)hipDeviceSynchronize();
        std::unique_lock<std::mutex> tg(e->slot_mu);
        for (Slot* sl : e->all_slots) {
            uint32_t f[4] = {0u, 0u, 0u, 0u};
            if (sl->sw_ready && sl->sw.flags && hipMemcpy(f, sl->sw.flags, sizeof(f), hipMemcpyDeviceToHost) == hipSuccess) t += f[1];
            if (sl->d_partials && hipMemcpy(f, partials_ticket(sl->d_partials) + 8, sizeof(f), hipMemcpyDeviceToHost) == hipSuccess) t += f[1];   // the fused path's short merge
        }
        for (int r = 0; r < kShardRing; ++r) {
            uint32_t f[4] = {0u, 0u, 0u, 0u};
            if (e->ring_d_partials[r] && hipMemcpy(f, partials_ticket(e->ring_d_partials[r]) + 8, sizeof(f), hipMemcpyDeviceToHost) == hipSuccess) t += f[1];
        }
        return t;
    }
    if (k == "stream_nt") return e->stream_nt.load();
    if (k == "fuse_merge") return e->fuse_merge.load();
    if (k == "query_args") return e->query_args.load();
    if (k == "done_flag") return e->done_flag.load();
    if (k == "merge_kway") return e->merge_kway.load();
    if (k == "merge_overlap_mb") return e->merge_overlap_mb.load();
    if (k == "batch_qfrag") return e->batch_qfrag.load();
    if (k == "overlap_scans") return (int64_t)e->st_overlap_scans.load();
    if (k == "scan_plain_mb") return e->scan_plain_mb.load();
    if (k == "scan_mirror") return e->scan_mirror.load();
    if (k == "mirror_scans") return (int64_t)e->st_mirror_scans.load();
    if (k == "mirror_scan_fallbacks") return (int64_t)e->st_mirror_fallbacks.load();
    if (k == "mirror_scan_unavailable") return (int64_t)e->st_mirror_unavailable.load();
    if (k == "mirror_share") return e->mirror_share.load();
    if (k == "mirror_passes") return (int64_t)e->st_mirror_passes.load();                    // scan launches over the mirror, whatever they carried
    if (k == "mirror_shared_passes") return (int64_t)e->st_mirror_shared_passes.load();      // ... of which with two or more queries
    if (k == "mirror_shared_queries") return (int64_t)e->st_mirror_shared_queries.load();    // queries answered by those
    if (k == "mirror_fill") return e->mirror_fill.load();
    if (k == "mirror_bits") return e->mirror_bits.load();
    if (k == "mirror8_passes") return (int64_t)e->st_mirror8_passes.load();              // passes over the 8-bit code mirror (lone or shared; also counted in "mirror_passes")
    if (k == "mirror8_fallbacks") return (int64_t)e->st_mirror8_fallbacks.load();        // 8-bit queries whose certificate failed (also counted in "mirror_scan_fallbacks")
    if (k == "mirror8_unavailable") return (int64_t)e->st_mirror8_unavailable.load();    // queries sent to bf16 because the code mirror could not be prepared
    if (k == "mirror8_conversions") return (int64_t)e->batch.conversions8.load();        // code mirror: conversions enqueued / rows converted so far
    if (k == "mirror8_rows_converted") return (int64_t)e->batch.rows8_converted.load();
    if (k == "mirror8_breaker_trips") return (int64_t)e->st_mirror8_breaker_trips.load();
    if (k == "mirror_fill_holds") return (int64_t)e->st_mirror_fill_holds.load();            // submits parked / held and blocking collects that held the parked set back ("mirror_fill" 1)
    if (k == "done_flag_waits") return (int64_t)e->st_flag_waits.load();
    if (k == "query_args_scans") return (int64_t)e->st_query_args.load();
    if (k == "merged_scans") return (int64_t)e->st_merged_scans.load();
    if (k == "batch_inline_retries") return (int64_t)e->st_batch_inline_retries.load();
    if (k == "retry_hint") return e->retry_hint.load();
    if (k == "batch_eps_measured") return e->batch_eps_measured.load();
    if (k == "batch_max_row_err_e9" || k == "batch_max_norm_e6") {   // the mirror's measured bounds (device words; a blocking read)
        unsigned int bits[2] = {0u, 0u};
        if (e->batch.d_maxnorm) {
            DeviceGuard g(e->device);
            (void)hipDeviceSynchronize();
            (void)hipMemcpy(bits, e->batch.d_maxnorm, sizeof(bits), hipMemcpyDeviceToHost);
        }
        float f[2];
        std::memcpy(f, bits, sizeof(f));
        return k == "batch_max_norm_e6" ? (int64_t)((double)f[0] * 1e6) : (int64_t)((double)f[1] * 1e9);
    }
    if (k == "mirror_rows_converted") return (int64_t)e->batch.rows_converted.load();   // bf16 mirror: rows converted so far / conversions enqueued
    if (k == "mirror_conversions") return (int64_t)e->batch.conversions.load();
    if (k == "compact_window_rows") return e->compact_window_rows.load();
    if (k == "remove_batches") return (int64_t)e->st_remove_batches.load();            // wax_hip_remove_batch calls that removed rows in one pass
    if (k == "remove_batch_rows") return (int64_t)e->st_remove_batch_rows.load();      // rows they removed
    if (k == "remove_batch_bytes_written") return (int64_t)e->st_remove_batch_bytes.load();   // device bytes their passes wrote (bounce writes included)
    if (k == "predicate_route") return e->predicate_route.load();
    if (k == "predicate_scan_min_permille") return e->predicate_scan_min_permille.load();
    if (k == "predicate_searches") return (int64_t)e->st_predicate_searches.load();          // wax_hip_search_predicate calls with a non-empty predicate
    if (k == "predicate_gather_searches") return (int64_t)e->st_predicate_gather.load();     // ... answered by gathering the passing rows
    if (k == "predicate_masked_scans") return (int64_t)e->st_predicate_masked.load();        // ... answered by the masked f32 scan
    if (k == "predicate_chunks_skipped") return (int64_t)e->st_predicate_skipped.load();     // chunks those scans did not load
    if (k == "predicate_mirror") return e->predicate_mirror.load();
    if (k == "predicate_mirror_scans") return (int64_t)e->st_predicate_mirror_scans.load();              // masked scans answered from the bf16 mirror under the certificate
    if (k == "predicate_mirror_fallbacks") return (int64_t)e->st_predicate_mirror_fallbacks.load();      // ... whose certificate failed: the masked f32 scan answered
    if (k == "predicate_mirror_unavailable") return (int64_t)e->st_predicate_mirror_unavailable.load();  // ... sent to the f32 scan because the mirror could not be prepared
    if (k == "attr_uploaded_rows") return (int64_t)e->st_attr_uploaded.load();               // rows of the attribute columns uploaded so far
    if (k == "attr_device_rows") return (int64_t)e->attr_cap;                                // rows the device columns are allocated for (0 = none)
    if (k == "idhash_rows_inserted") return (int64_t)e->st_idhash_rows.load();
    if (k == "batch_min") return e->batch_min.load();
    if (k == "batch_mode") return e->batch_mode.load();
    if (k == "batch_rega") return e->batch_rega.load();
    if (k == "batch_dyn_tail") return e->batch_dyn_tail.load();
    if (k == "batch_in_wait") return e->batch_in_wait.load();
    if (k == "batch_host_multi") return e->batch_host_multi.load();
    if (k == "batch_slab_mb") return e->batch_slab_mb.load();
    if (k == "batch_growth") return e->batch_growth.load();
    if (k == "batch_first") return e->batch_first.load();
    if (k == "batch_onepass") return e->batch_onepass.load();
    if (k == "batch_onepass_tiles") return e->batch_onepass_tiles.load();
    if (k == "batch_kp_fused") return e->batch_kp_fused.load();
    if (k == "batch_survivors") return e->batch_survivors.load();
    if (k == "batch_sample_div") return e->batch_sample_div.load();
    if (k == "batch_workspaces") return e->bctx_max;
    if (k == "batch_max_k") return kBatchMaxK;
    if (k == "onepass_queries") return (int64_t)e->st_onepass_queries.load();
    if (k == "scan_chain") return e->scan_chain.load();
    if (k == "share_timing") return e->share_timing.load();
    if (k == "batch_retry") return e->batch_retry.load();
    if (k == "batch_retries") return (int64_t)e->st_batch_retries.load();
    if (k == "batch_multi") return e->batch_multi.load();
    if (k == "batch_multi_passes") return (int64_t)e->st_multi_passes.load();
    if (k == "batch_multi_queries") return (int64_t)e->st_multi_queries.load();
    if (k == "batch_multi_group") return (int64_t)scan_multi_group(e->dims, 10);        // queries per shared exact pass, k <= 60 (64-slot lists)
    if (k == "batch_multi_group_big") return (int64_t)scan_multi_group(e->dims, 192);   // ... k <= 192 (256-slot lists)
    if (k == "filter_device_min") return e->filter_device_min.load();
    if (k == "filter_device_searches") return (int64_t)e->st_filter_device.load();
    if (k == "filter_batch") return e->filter_batch.load();
    if (k == "filter_batch_queries") return (int64_t)e->st_filter_batch_queries.load();
    if (k == "filter_batch_fallbacks") return (int64_t)e->st_filter_batch_fallbacks.load();
    if (k == "predicate_batch_rows") return e->predicate_batch_rows.load();
    if (k == "predicate_batch_queries") return (int64_t)e->st_predicate_batch_queries.load();   // non-empty predicates answered by the batched gather pass
    if (k == "predicate_batch_classes") return (int64_t)e->st_predicate_batch_classes.load();   // (list, predicate) entries with a predicate that pass built
    if (k == "search_many") return e->search_many.load();
    if (k == "search_many_max_rows") return e->search_many_max_rows.load();
    if (k == "search_many_pooled") return (int64_t)e->st_many_pooled.load();   // pairs of wax_hip_search_many answered by its pooled launch
    if (k == "search_many_looped") return (int64_t)e->st_many_looped.load();   // ... by the single-query search under the call's lock
    if (k == "search_many_masked") return (int64_t)e->st_many_masked.load();   // ... of the pooled ones: by a masked group (a non-empty predicate evaluated on the device)
    if (k == "batch_queries") return (int64_t)e->st_batch_queries.load();
    if (k == "batch_fallbacks") return (int64_t)e->st_batch_fallbacks.load();
    if (k == "slots") return e->max_slots;
    if (k == "streams") return e->n_streams;
    if (k == "variant_count") return scan_variant_count(e->dims);
    if (k == "scan_grid") return scan_grid_for((uint32_t)e->count, e->dims, (int)e->variant.load(), (int)e->grid_blocks.load());
    if (k == "fused_max_k") return FUSED_MAX_K;
    if (k == "store_ptr") return (int64_t)(uintptr_t)e->d_store;   // diagnosis: where the slab sits (tools/bimodal_probe.py)
    return -1;
}

int wax_hip_time_scan_kernel(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, uint32_t iters,
                             double* out_avg_ms) {
    if (!e || !out_avg_ms || !query) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    SHARDED_UNSUPPORTED(e, "wax_hip_time_scan_kernel");
    if (dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));
    if (iters == 0) iters = 1;
    DeviceGuard g(e->device);
    e->lock.lock_shared(holding(e) > 0);
    { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) { e->lock.unlock_shared(); return frc; } }
    Slot* s = nullptr;
    int rc = WAX_HIP_OK;
    do {
        if (e->count == 0) { rc = fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is empty"); break; }
        const int limit = clamp_topk(top_k);
        const int k_eff = (uint64_t)limit < e->count ? limit : (int)e->count;
        if (k_eff > FUSED_MAX_K) { rc = fail(WAX_HIP_ERR_INVALID_ARGUMENT, "time_scan_kernel: top_k must be <= 192"); break; }
        rc = acquire_slot(e, &s);
        if (rc != WAX_HIP_OK) break;
        std::memcpy(s->h_query, query, (size_t)dims * sizeof(float));
        ScanArgs a{};
        a.store = e->d_store; a.query = s->d_query; a.partials = s->d_partials; a.dist_out = nullptr;
        a.n_rows = (uint32_t)e->count; a.row_base = (uint32_t)e->row_base; a.dims = e->dims; a.k = k_eff;
        a.q_norm = query_norm(query, dims);
        const int cap = wave_list_cap(k_eff);
        hipError_t err = hipMemcpyAsync(s->d_query, s->h_query, (size_t)dims * sizeof(float), hipMemcpyHostToDevice, s->stream);
        int grid = 0;
        for (int wu = 0; wu < 2 && err == hipSuccess; ++wu)
            err = launch_scan(a, e->metric, (int)e->variant.load(), cap, false, (int)e->grid_blocks.load(), s->stream, &grid);
        if (err == hipSuccess) err = hipEventRecord(s->ev0, s->stream);
        for (uint32_t i = 0; i < iters && err == hipSuccess; ++i)
            err = launch_scan(a, e->metric, (int)e->variant.load(), cap, false, (int)e->grid_blocks.load(), s->stream, &grid);
        if (err == hipSuccess) err = hipEventRecord(s->ev1, s->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(s->stream);
        float ms = 0.f;
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, s->ev0, s->ev1);
        if (err != hipSuccess) { rc = fail(WAX_HIP_ERR_INTERNAL, std::string("time_scan_kernel: ") + hipGetErrorString(err)); break; }
        *out_avg_ms = (double)ms / (double)iters;
    } while (0);
    if (s) release_slot(e, s);
    e->lock.unlock_shared();
    return rc;
}

int wax_hip_time_stream_read(wax_hip_engine* e, uint32_t iters, double* out_avg_ms) {
    if (!e || !out_avg_ms) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    SHARDED_UNSUPPORTED(e, "wax_hip_time_stream_read");
    if (iters == 0) iters = 1;
    DeviceGuard g(e->device);
    e->lock.lock_shared(holding(e) > 0);
    { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) { e->lock.unlock_shared(); return frc; } }
    Slot* s = nullptr;
    int rc = WAX_HIP_OK;
    do {
        const uint64_t bytes = (e->count * (uint64_t)e->dims * 4ull) & ~15ull;
        if (bytes == 0) { rc = fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is empty"); break; }
        rc = acquire_slot(e, &s);
        if (rc != WAX_HIP_OK) break;
        int grid = (int)e->grid_blocks.load();
        if (grid <= 0) grid = 2048;
        if (grid > MAX_GRID_BLOCKS) grid = MAX_GRID_BLOCKS;
        const int nt = (int)e->stream_nt.load();
        hipError_t err = hipSuccess;
        for (int wu = 0; wu < 2 && err == hipSuccess; ++wu) err = launch_stream_read(e->d_store, bytes, nt, grid, e->d_sink, s->stream);
        if (err == hipSuccess) err = hipEventRecord(s->ev0, s->stream);
        for (uint32_t i = 0; i < iters && err == hipSuccess; ++i) err = launch_stream_read(e->d_store, bytes, nt, grid, e->d_sink, s->stream);
        if (err == hipSuccess) err = hipEventRecord(s->ev1, s->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(s->stream);
        float ms = 0.f;
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, s->ev0, s->ev1);
        if (err != hipSuccess) { rc = fail(WAX_HIP_ERR_INTERNAL, std::string("time_stream_read: ") + hipGetErrorString(err)); break; }
        *out_avg_ms = (double)ms / (double)iters;
    } while (0);
    if (s) release_slot(e, s);
    e->lock.unlock_shared();
    return rc;
}


// Diagnostic read-out of the 8-bit code mirror as the device holds it (tests/test_mirror8_edges_gpu.py): a copy, never a build or a
// refresh, no counter and no breaker state touched. Refused unless the code mirror is valid, so it never hands out rows that are not coded.
int wax_hip_mirror8_snapshot(wax_hip_engine* e, uint64_t first_row, uint64_t n_rows, uint8_t* out_codes, float* out_meta,
                             float* out_max_norm, uint64_t* out_rows_coded) {
    if (!e || !out_max_norm || !out_rows_coded || (n_rows > 0 && (!out_codes || !out_meta))) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    SHARDED_UNSUPPORTED(e, "wax_hip_mirror8_snapshot");
    DeviceGuard g(e->device);
    ReadGuard rg(e);
    BatchMirror& b = e->batch;
    std::unique_lock<std::mutex> mg(b.mu8);
    if (!b.c8_valid.load(std::memory_order_acquire) || b.d_c8 == nullptr || b.d_c8_meta == nullptr || b.d_c8_max == nullptr || b.c8_cap < e->capacity)
        return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror8_snapshot: the code mirror is absent or not valid");
    const uint64_t rows = b.rows8.load();
    if (first_row > rows || n_rows > rows - first_row)
        return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror8_snapshot: rows [" + std::to_string(first_row) + ", " + std::to_string(first_row) + " + " +
                                                  std::to_string(n_rows) + ") exceed the " + std::to_string(rows) + " coded rows");
    if (b.ev8_pending) HIP_TRY(hipEventSynchronize(b.ev8_ready), WAX_HIP_ERR_INTERNAL, "code mirror ready wait");
    const size_t D = e->dims;
    unsigned int max_bits = 0u;
    HIP_TRY(hipMemcpy(&max_bits, b.d_c8_max, sizeof(max_bits), hipMemcpyDeviceToHost), WAX_HIP_ERR_INTERNAL, "mirror8_snapshot copy");
    if (n_rows > 0) {
        HIP_TRY(hipMemcpy(out_codes, b.d_c8 + first_row * D, (size_t)n_rows * D, hipMemcpyDeviceToHost), WAX_HIP_ERR_INTERNAL, "mirror8_snapshot copy");
        HIP_TRY(hipMemcpy(out_meta, b.d_c8_meta + 2 * first_row, (size_t)n_rows * 2 * sizeof(float), hipMemcpyDeviceToHost), WAX_HIP_ERR_INTERNAL, "mirror8_snapshot copy");
    }
    std::memcpy(out_max_norm, &max_bits, sizeof(float));
    *out_rows_coded = rows;
    return WAX_HIP_OK;
}

// Diagnostic read-out of the keys of the 8-bit pass (tests/test_mirror8_mfma_gpu.py): the lower bound the lone scan computes for
// `query` at every coded row, by the scan's own body. Like the snapshot: never a build or a refresh, no counter and no breaker state
// touched, refused unless the code mirror is valid. No product path calls it.
int wax_hip_mirror8_keys(wax_hip_engine* e, const float* query, float* out_keys, uint64_t n_keys) {
    if (!e || !query || !out_keys) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    SHARDED_UNSUPPORTED(e, "wax_hip_mirror8_keys");
    DeviceGuard g(e->device);
    ReadGuard rg(e);
    BatchMirror& b = e->batch;
    std::unique_lock<std::mutex> mg(b.mu8);
    if (!b.c8_valid.load(std::memory_order_acquire) || b.d_c8 == nullptr || b.d_c8_meta == nullptr || b.d_c8_max == nullptr || b.c8_cap < e->capacity)
        return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror8_keys: the code mirror is absent or not valid");
    const uint64_t rows = b.rows8.load();
    if (rows == 0 || rows > e->count || n_keys != rows)
        return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror8_keys: out_keys holds " + std::to_string(n_keys) + " keys, the code mirror " + std::to_string(rows) + " rows");
    if (!mirror_scan_supported(e->dims, e->metric)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror8_keys: no 8-bit pass at this dimension and metric");
    if (b.ev8_pending) HIP_TRY(hipEventSynchronize(b.ev8_ready), WAX_HIP_ERR_INTERNAL, "code mirror ready wait");
    MirrorScanArgs m{};
    m.n_rows = (uint32_t)rows;
    m.row_base = (uint32_t)e->row_base;
    m.dims = e->dims;
    m.k = 1;
    m.kpad = 1;
    m.q_norm = query_norm(query, e->dims);
    float* d_keys = nullptr;
    HIP_TRY(hipMalloc(&d_keys, (size_t)rows * sizeof(float)), WAX_HIP_ERR_INTERNAL, "mirror8_keys allocation");
    hipError_t err = launch_mirror8_keys(m, b.d_c8, b.d_c8_meta, query, e->metric, (int)e->grid_blocks.load(), d_keys, nullptr);
    if (err == hipSuccess) err = hipMemcpy(out_keys, d_keys, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d_keys);
    HIP_TRY(err, WAX_HIP_ERR_INTERNAL, "mirror8_keys");
    return WAX_HIP_OK;
}
