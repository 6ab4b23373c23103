// api_predicate.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: per-row attributes (set / get) and the predicate search (DESIGN 2, 4.5; passesFrameFilter, UnifiedSearch.swift:1241-1258)

// ---- per-row attributes ---------------------------------------------------------

int wax_hip_set_attributes(wax_hip_engine* e, const uint64_t* frame_ids, const int64_t* timestamps, const uint32_t* flags, uint64_t n,
                           uint64_t* out_applied) {
    if (out_applied) *out_applied = 0;
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (n == 0) return WAX_HIP_OK;
    if (!frame_ids) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "setAttributes: null input");
    if (e->sh) return sh_set_attributes(e, frame_ids, timestamps, flags, n, out_applied);
    REFUSE_IF_HOLDING(e);
    WriteGuard w(e->lock);
    uint64_t applied = 0, lowest = UINT64_MAX;
    for (uint64_t i = 0; i < n; ++i) {
        const int64_t r = e->idmap.find(frame_ids[i]);
        if (r < 0) continue;                                   // a frame without a vector has no row to describe
        ++applied;
        if (!timestamps && !flags) continue;
        if (e->attr_ts.size() <= (uint64_t)r) {                // the columns end below this row: everything up to it was (0, 0)
            e->attr_ts.resize((size_t)e->count, 0);
            e->attr_flags.resize((size_t)e->count, 0u);
        }
        if (timestamps) e->attr_ts[(size_t)r] = timestamps[i];  // in call order: the last entry of a repeated id wins
        if (flags) e->attr_flags[(size_t)r] = flags[i];
        if ((uint64_t)r < lowest) lowest = (uint64_t)r;
    }
    if (lowest != UINT64_MAX) attr_note_moved(e, lowest);
    if (out_applied) *out_applied = applied;
    return WAX_HIP_OK;
}

int wax_hip_get_attributes(wax_hip_engine* e, const uint64_t* frame_ids, uint64_t n, int64_t* out_timestamps, uint32_t* out_flags,
                           uint8_t* out_found) {
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (n == 0) return WAX_HIP_OK;
    if (!frame_ids) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "getAttributes: null input");
    if (e->sh) return sh_get_attributes(e, frame_ids, n, out_timestamps, out_flags, out_found);
    e->lock.lock_shared(holding(e) > 0);
    struct Unlock { RWLock& l; ~Unlock() { l.unlock_shared(); } } unlock{e->lock};
    const uint64_t na = e->attr_ts.size();
    for (uint64_t i = 0; i < n; ++i) {
        const int64_t r = e->idmap.find(frame_ids[i]);
        const bool set = r >= 0 && (uint64_t)r < na;
        if (out_timestamps) out_timestamps[i] = set ? e->attr_ts[(size_t)r] : 0;
        if (out_flags) out_flags[i] = set ? e->attr_flags[(size_t)r] : 0u;
        if (out_found) out_found[i] = r >= 0 ? 1 : 0;
    }
    return WAX_HIP_OK;
}

// The device columns of the store as it is now (shared lock held; pending rows flushed), or two null pointers for a store whose
// host columns are empty (never set, or dropped by deserialize): the kernel then reads every row as (0, 0) and nothing is allocated.
// Concurrent predicate searches serialise here; what is uploaded is rows [lowest changed or first appended, count).
static int ensure_attrs(wax_hip_engine* e, hipStream_t st, const int64_t** d_ts, const uint32_t** d_flags) {
    *d_ts = nullptr; *d_flags = nullptr;
    std::unique_lock<std::mutex> g(e->attr_mu);
    const uint64_t na = e->attr_ts.size(), count = e->count;
    if (na == 0) return WAX_HIP_OK;
    if (e->attr_cap < count) {
        // growth: columns of the store's capacity; the rows that were up to date are kept (a device copy), the rest is uploaded below
        const uint64_t cap = e->capacity > count ? e->capacity : count;
        const uint64_t keep = std::min(std::min(e->attr_dev_rows, e->attr_stale_from), e->attr_cap);
        int64_t* nt = nullptr;
        uint32_t* nf = nullptr;
        HIP_TRY(hipMalloc(&nt, (size_t)cap * sizeof(int64_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate the timestamp column");
        hipError_t err = hipMalloc(&nf, (size_t)cap * sizeof(uint32_t));
        if (err == hipSuccess && keep > 0) err = hipMemcpyAsync(nt, e->d_attr_ts, (size_t)keep * sizeof(int64_t), hipMemcpyDeviceToDevice, st);
        if (err == hipSuccess && keep > 0) err = hipMemcpyAsync(nf, e->d_attr_flags, (size_t)keep * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        if (err != hipSuccess) { (void)hipFree(nt); (void)hipFree(nf); return fail(WAX_HIP_ERR_ALLOC, std::string("Failed to allocate the flag column: ") + hipGetErrorString(err)); }
        (void)hipFree(e->d_attr_ts); (void)hipFree(e->d_attr_flags);
        e->d_attr_ts = nt; e->d_attr_flags = nf; e->attr_cap = cap; e->attr_dev_rows = keep;
    }
    const uint64_t from = std::min(std::min(e->attr_dev_rows, e->attr_stale_from), count);
    if (from < count) {
        const uint64_t host_end = std::min(na, count);         // rows behind the host columns are (0, 0)
        if (from < host_end) {
            // pageable sources: the runtime stages them before returning
            HIP_TRY(hipMemcpyAsync(e->d_attr_ts + from, e->attr_ts.data() + from, (size_t)(host_end - from) * sizeof(int64_t), hipMemcpyHostToDevice, st),
                    WAX_HIP_ERR_INTERNAL, "timestamp upload");
            HIP_TRY(hipMemcpyAsync(e->d_attr_flags + from, e->attr_flags.data() + from, (size_t)(host_end - from) * sizeof(uint32_t), hipMemcpyHostToDevice, st),
                    WAX_HIP_ERR_INTERNAL, "flag upload");
        }
        const uint64_t z0 = std::max(from, host_end);
        if (z0 < count) {
            HIP_TRY(hipMemsetAsync(e->d_attr_ts + z0, 0, (size_t)(count - z0) * sizeof(int64_t), st), WAX_HIP_ERR_INTERNAL, "timestamp fill");
            HIP_TRY(hipMemsetAsync(e->d_attr_flags + z0, 0, (size_t)(count - z0) * sizeof(uint32_t), st), WAX_HIP_ERR_INTERNAL, "flag fill");
        }
        HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "attribute upload failed on device");   // other workspaces' streams read the columns next
        e->st_attr_uploaded += count - from;
    }
    e->attr_dev_rows = count;
    e->attr_stale_from = UINT64_MAX;
    *d_ts = e->d_attr_ts; *d_flags = e->d_attr_flags;
    return WAX_HIP_OK;
}

// ---- predicate search -----------------------------------------------------------

static inline bool predicate_is_empty(const wax_hip_row_predicate* p) {
    return p == nullptr || (p->has_after == 0 && p->has_before == 0 && p->deny_flags == 0u);
}
static inline bool predicate_passes(const wax_hip_row_predicate& p, int64_t ts, uint32_t fl) {
    return !(p.has_after != 0 && ts < p.after) && !(p.has_before != 0 && ts >= p.before) && (fl & p.deny_flags) == 0u;
}

static int grow_filter_lists(FilterWork& f, uint64_t m) {
    if (f.cap >= m) return WAX_HIP_OK;
    uint64_t cap = 1024;
    while (cap < m) cap *= 2;
    uint64_t c1 = f.cap, c2 = f.cap, c3 = f.cap;
    int grc = grow_dev(&f.d_rows, &c1, cap, sizeof(uint32_t), "Failed to allocate allowed-row list");
    if (grc == WAX_HIP_OK) grc = grow_dev(&f.d_ids, &c2, cap, sizeof(uint64_t), "Failed to allocate allowed-id list");
    if (grc == WAX_HIP_OK) grc = grow_dev(&f.d_dist, &c3, cap, sizeof(float), "Failed to allocate allowed-row distances");
    f.cap = grc == WAX_HIP_OK ? cap : 0;
    return grc;
}

// Gather route, from the compact list on: f.d_rows / f.d_ids hold the m passing rows ascending. Exact f32 distances with scan_kernel's
// lane mapping and summation order, then the general selection — what search_filtered_locked does behind its allow-list.
static int predicate_gather_tail(wax_hip_engine* e, FilterWork& f, const float* query, uint32_t dims, uint64_t m, int kpad,
                                 uint64_t* out_ids, float* out_scores, uint32_t out_capacity, uint32_t* out_n) {
    hipStream_t st = f.stream;
    const int k_eff = (uint64_t)kpad < m ? kpad : (int)m;
    const float qn = query_norm(query, dims);
    HIP_TRY(hipMemcpyAsync(f.d_query, query, (size_t)dims * sizeof(float), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "query upload");
    HIP_TRY(hipMemcpyAsync(f.d_qnorm, &qn, sizeof(float), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "query norm upload");
    RescoreArgs r{};
    r.store = e->d_store; r.queries = f.d_query; r.q_norm = f.d_qnorm; r.rows = f.d_rows; r.dist_out = f.d_dist;
    r.n_rows = (uint32_t)e->count; r.row_base = 0; r.dims = dims; r.nq = 1; r.cand_cap = 0; r.kp = (int)m;
    HIP_TRY(launch_rescore(r, e->metric, st), WAX_HIP_ERR_INTERNAL, "distance kernel launch");
    // keys of the compact list carry the POSITION in it; positions ascend with rows, so ties order as everywhere else
    HIP_TRY(launch_select_general(f.d_dist, (uint32_t)m, 0u, k_eff, k_eff, f.d_ids, f.sw, f.d_hits, st), WAX_HIP_ERR_INTERNAL, "select kernel launch");
    HIP_TRY(hipMemcpyAsync(f.h_hits, f.d_hits, (size_t)k_eff * sizeof(wax_hip_hit), hipMemcpyDeviceToHost, st), WAX_HIP_ERR_INTERNAL, "hits download");
    HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "predicate search failed on device");
    const int rc = hits_to_results(e->metric, f.h_hits, (uint32_t)k_eff, out_ids, out_scores, out_capacity, out_n);
    if (rc != WAX_HIP_OK) return rc;
    e->st_searches++;
    e->st_predicate_gather++;
    e->st_rows += m;
    e->st_bytes += m * (uint64_t)e->dims * 4ull;
    return WAX_HIP_OK;
}

// One query with a non-empty predicate (and perhaps an allow-list), on a pooled filter workspace; the caller holds the shared lock and
// has flushed pending rows. *out_n = results written (before any score cut).
static int search_predicate_locked(wax_hip_engine* e, const float* query, uint32_t dims, int kpad, int has_allow, const uint64_t* allow_frame_ids,
                                   uint64_t n_allow, const wax_hip_row_predicate& pred, uint64_t* out_ids, float* out_scores,
                                   uint32_t out_capacity, uint32_t* out_n) {
    *out_n = 0;
    e->st_predicate_searches++;
    if (e->count == 0 || (has_allow && n_allow == 0)) return WAX_HIP_OK;
    if (e->row_base + e->count > 0x100000000ull) return fail(WAX_HIP_ERR_CAPACITY, "row_base + count exceeds UInt32 row indices");
    FilterWork* fp = nullptr;
    { const int arc = acquire_filter_work(e, &fp); if (arc != WAX_HIP_OK) return arc; }
    struct Release { wax_hip_engine* e; FilterWork* f; ~Release() { (void)hipStreamSynchronize(f->stream); release_filter_work(e, f); } } release{e, fp};
    FilterWork& f = *fp;
    hipStream_t st = f.stream;
    const uint32_t count = (uint32_t)e->count;
    const int64_t dev_min = e->filter_device_min.load();
    if (has_allow && !(dev_min >= 0 && n_allow >= (uint64_t)dev_min)) {
        // short allow-list: its rows are probed on the host, where the authoritative attribute columns are too — the predicate is
        // evaluated here on those few rows and the survivors take the gather route
        const uint64_t na = e->attr_ts.size();
        std::vector<uint32_t> rows;
        rows.reserve((size_t)n_allow);
        for (uint64_t i = 0; i < n_allow; ++i) {
            const int64_t r = e->idmap.find(allow_frame_ids[i]);
            if (r < 0) continue;
            const bool set = (uint64_t)r < na;
            if (predicate_passes(pred, set ? e->attr_ts[(size_t)r] : 0, set ? e->attr_flags[(size_t)r] : 0u)) rows.push_back((uint32_t)r);
        }
        std::sort(rows.begin(), rows.end());
        rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
        const uint64_t m = rows.size();
        if (m == 0) return WAX_HIP_OK;
        std::vector<uint64_t> ids((size_t)m);
        for (uint64_t i = 0; i < m; ++i) ids[i] = e->ids[rows[i]];
        { const int grc = grow_filter_lists(f, m); if (grc != WAX_HIP_OK) return grc; }
        HIP_TRY(hipMemcpyAsync(f.d_rows, rows.data(), (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "row list upload");
        HIP_TRY(hipMemcpyAsync(f.d_ids, ids.data(), (size_t)m * sizeof(uint64_t), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "id list upload");
        HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "row list upload");
        return predicate_gather_tail(e, f, query, dims, m, kpad, out_ids, out_scores, out_capacity, out_n);
    }
    // ---- the row bitmap: [allow-list probe,] attributes ----
    const int64_t* d_ts = nullptr;
    const uint32_t* d_fl = nullptr;
    { const int arc = ensure_attrs(e, st, &d_ts, &d_fl); if (arc != WAX_HIP_OK) return arc; }
    const uint64_t n_words = ((uint64_t)count + 31) / 32, n_blocks = filter_bitmap_blocks(count);
    int grc = grow_dev(&f.d_bitmap, &f.bitmap_words, n_words, sizeof(uint32_t), "Failed to allocate row bitmap");
    if (grc == WAX_HIP_OK) grc = grow_dev(&f.d_block_sum, &f.block_cap, n_blocks, sizeof(uint32_t), "Failed to allocate bitmap offsets");
    if (grc != WAX_HIP_OK) return grc;
    if (!f.h_pred_counts)   // each word on its own test: a call that got one and was refused the other must not leave the next call a null pointer
        HIP_TRY(hipHostMalloc(&f.h_pred_counts, 2 * sizeof(uint32_t), hipHostMallocDefault), WAX_HIP_ERR_ALLOC, "Failed to allocate predicate counters");
    if (!f.d_pred_counts)
        HIP_TRY(hipMalloc(&f.d_pred_counts, 2 * sizeof(uint32_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate predicate counters");
    if (has_allow) {
        { const int hrc = ensure_idhash(e, st); if (hrc != WAX_HIP_OK) return hrc; }
        grc = grow_dev(&f.d_allow, &f.allow_cap, n_allow, sizeof(uint64_t), "Failed to allocate allow-list");
        if (grc != WAX_HIP_OK) return grc;
        HIP_TRY(hipMemcpyAsync(f.d_allow, allow_frame_ids, (size_t)n_allow * sizeof(uint64_t), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "allow-list upload");
        HIP_TRY(launch_allow_probe(f.d_allow, n_allow, e->d_ids, count, e->idhash.d_table, e->idhash.slots, f.d_bitmap, nullptr, nullptr, st),
                WAX_HIP_ERR_INTERNAL, "allow-list probe launch");
        e->st_filter_device++;
    }
    const bool scan_shape = scan_masked_dims(dims) && kpad <= FUSED_MAX_K && e->force_general.load() == 0;   // kpad = clamp(top_k): top_k > 192 gathers
    const uint32_t chunk_rows = scan_shape ? scan_masked_chunk_rows(dims) : 0u;
    AttrMaskArgs ma{};
    ma.ts = d_ts; ma.flags = d_fl; ma.bitmap = f.d_bitmap; ma.counts = f.d_pred_counts; ma.n_rows = count; ma.chunk_rows = chunk_rows;
    ma.and_bitmap = has_allow ? 1 : 0;
    ma.has_after = pred.has_after != 0; ma.has_before = pred.has_before != 0; ma.after = pred.after; ma.before = pred.before; ma.deny_flags = pred.deny_flags;
    HIP_TRY(hipMemsetAsync(f.d_pred_counts, 0, 2 * sizeof(uint32_t), st), WAX_HIP_ERR_INTERNAL, "predicate counters");
    HIP_TRY(launch_attr_mask(ma, st), WAX_HIP_ERR_INTERNAL, "attribute mask launch");
    HIP_TRY(hipMemcpyAsync(f.h_pred_counts, f.d_pred_counts, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st), WAX_HIP_ERR_INTERNAL, "row count download");
    HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "attribute mask failed on device");
    const uint64_t m = f.h_pred_counts[0], live_chunks = f.h_pred_counts[1];
    if (m == 0) return WAX_HIP_OK;
    // ---- route ----
    const int64_t route = e->predicate_route.load();
    const bool masked = scan_shape && route != 1 &&
                        (route == 2 || m * 1000ull >= (uint64_t)e->predicate_scan_min_permille.load() * (uint64_t)count);
    if (!masked) {
        { const int lrc = grow_filter_lists(f, m); if (lrc != WAX_HIP_OK) return lrc; }
        HIP_TRY(launch_bitmap_offsets(f.d_bitmap, count, f.d_block_sum, f.d_total, st), WAX_HIP_ERR_INTERNAL, "bitmap offsets launch");
        HIP_TRY(launch_allow_emit(f.d_bitmap, count, f.d_block_sum, e->d_ids, f.d_rows, f.d_ids, st), WAX_HIP_ERR_INTERNAL, "row compaction launch");
        return predicate_gather_tail(e, f, query, dims, m, kpad, out_ids, out_scores, out_capacity, out_n);
    }
    // ---- masked scan: the f32 scan's rows, loads and arithmetic; chunks without a passing row are not read ----
    if (!f.d_partials) {
        HIP_TRY(hipMalloc(&f.d_partials, kPartialsBytes), WAX_HIP_ERR_ALLOC, "Failed to allocate top-k stage buffer");
        HIP_TRY(hipMemsetAsync(partials_ticket(f.d_partials), 0, 128, st), WAX_HIP_ERR_INTERNAL, "top-k stage buffer");
    }
    const int k_eff = (uint64_t)kpad < m ? kpad : (int)m;
    const int cap = k_eff <= 64 ? 128 : 256;
    HIP_TRY(hipMemcpyAsync(f.d_query, query, (size_t)dims * sizeof(float), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "query upload");
    MaskedScanArgs a{};
    a.store = e->d_store; a.query = f.d_query; a.bitmap = f.d_bitmap; a.partials = f.d_partials;
    a.n_rows = count; a.row_base = (uint32_t)e->row_base; a.dims = dims; a.k = k_eff; a.q_norm = query_norm(query, dims);
    int grid = 0;
    HIP_TRY(launch_scan_masked(a, e->metric, cap, (int)e->grid_blocks.load(), st, &grid), WAX_HIP_ERR_INTERNAL, "masked scan launch");
    // the second-launch merge of enqueue_scan: the short selection for 64 < k <= 192 with the wave-list merge behind it, gated
    uint32_t* short_flags = nullptr;
    if (e->select_short.load() != 0 && k_eff > SCAN_KWAY_MAX_K && select_short_viable(k_eff, grid, k_eff)) {
        short_flags = partials_ticket(f.d_partials) + 8;
        HIP_TRY(launch_select_short(f.d_partials, (uint32_t)grid, (uint32_t)k_eff, k_eff, k_eff, e->d_ids, a.row_base, a.n_rows, short_flags, f.d_hits, st),
                WAX_HIP_ERR_INTERNAL, "short merge launch");
    }
    HIP_TRY(launch_merge_keys(f.d_partials, (uint32_t)grid * (uint32_t)k_eff, k_eff, k_eff, e->d_ids, a.row_base, a.n_rows, f.d_hits, cap, st, short_flags),
            WAX_HIP_ERR_INTERNAL, "merge kernel launch");
    HIP_TRY(hipMemcpyAsync(f.h_hits, f.d_hits, (size_t)k_eff * sizeof(wax_hip_hit), hipMemcpyDeviceToHost, st), WAX_HIP_ERR_INTERNAL, "hits download");
    HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "predicate search failed on device");
    const int rc = hits_to_results(e->metric, f.h_hits, (uint32_t)k_eff, out_ids, out_scores, out_capacity, out_n);
    if (rc != WAX_HIP_OK) return rc;
    const uint64_t n_chunks = ((uint64_t)count + chunk_rows - 1) / chunk_rows;
    e->st_searches++;
    e->st_predicate_masked++;
    e->st_predicate_skipped += n_chunks - live_chunks;
    e->st_rows += live_chunks * chunk_rows;                                 // what was actually read: every row of a chunk that holds a passing one
    e->st_bytes += live_chunks * chunk_rows * (uint64_t)e->dims * 4ull;
    return WAX_HIP_OK;
}

int wax_hip_search_predicate(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, int has_allow,
                             const uint64_t* allow_frame_ids, uint64_t n_allow, int has_min_score, float min_score,
                             const wax_hip_row_predicate* pred, uint64_t* out_ids, float* out_scores, uint32_t out_capacity,
                             uint32_t* out_count) {
    if (out_count) *out_count = 0;
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (!query || !out_count || ((!out_ids || !out_scores) && out_capacity)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (has_allow && n_allow > 0 && !allow_frame_ids) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "allow-list is null");
    if (predicate_is_empty(pred))   // nothing to test per row: the filtered search (and, without a list, the ordinary scan) as it is
        return wax_hip_search_filtered(e, query, dims, top_k, has_allow, allow_frame_ids, n_allow, has_min_score, min_score, out_ids, out_scores,
                                       out_capacity, out_count);
    if (e->sh) return sh_search_predicate(e, query, dims, top_k, has_allow, allow_frame_ids, n_allow, has_min_score, min_score, pred, out_ids,
                                          out_scores, out_capacity, out_count);
    if (dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));
    uint32_t n = 0;
    {
        DeviceGuard g(e->device);
        e->lock.lock_shared(holding(e) > 0);
        struct Unlock { RWLock& l; ~Unlock() { l.unlock_shared(); } } unlock{e->lock};
        { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return frc; }
        const int rc = search_predicate_locked(e, query, dims, clamp_topk(top_k), has_allow, allow_frame_ids, n_allow, *pred, out_ids, out_scores,
                                               out_capacity, &n);
        if (rc != WAX_HIP_OK) return rc;
    }
    if (has_min_score) {  // `score < minScore` drops a candidate (UnifiedSearch.swift:1248); results are best-first
        uint32_t keep = 0;
        for (uint32_t i = 0; i < n; ++i)
            if (!(out_scores[i] < min_score)) { out_ids[keep] = out_ids[i]; out_scores[keep] = out_scores[i]; ++keep; }
        n = keep;
    }
    *out_count = n;
    return WAX_HIP_OK;
}
