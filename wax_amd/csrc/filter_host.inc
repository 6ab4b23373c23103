// filter_host.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: the filtered searches, host side (SURVEY 8f-4; DESIGN 4.5; passesFrameFilter, UnifiedSearch.swift:1241-1258) — one query with an
// allow-list and / or a row predicate (one locked body, built from the steps below), the predicate search as a ticket
// (wax_hip_search_predicate_submit: the routing is submit_impl's, api_search.inc), and the batched form (a list, a predicate and a
// cut per query)

// ---- the steps --------------------------------------------------------------------

static inline bool predicate_is_empty(const wax_hip_row_predicate* p) {
    return p == nullptr || (p->has_after == 0 && p->has_before == 0 && p->deny_flags == 0u);
}
static inline bool predicate_passes(const wax_hip_row_predicate& p, int64_t ts, uint32_t fl) {
    return !(p.has_after != 0 && ts < p.after) && !(p.has_before != 0 && ts >= p.before) && (fl & p.deny_flags) == 0u;
}

// A row predicate with the values of its unused bounds set to 0: two pairs whose predicates test the same thing compare equal.
static inline wax_hip_row_predicate normalised_predicate(const wax_hip_row_predicate* p) {
    wax_hip_row_predicate r{};
    if (!p) return r;
    r.has_after = p->has_after != 0; r.after = r.has_after ? p->after : 0;
    r.has_before = p->has_before != 0; r.before = r.has_before ? p->before : 0;
    r.deny_flags = p->deny_flags;
    return r;
}

// `score < minScore` drops a candidate (UnifiedSearch.swift:1248); results are best-first. A NaN cut keeps everything.
static inline void apply_min_score(float cut, uint64_t* ids, float* scores, uint32_t* n) {
    uint32_t keep = 0;
    for (uint32_t i = 0; i < *n; ++i)
        if (!(scores[i] < cut)) { ids[keep] = ids[i]; scores[keep] = scores[i]; ++keep; }
    *n = keep;
}

// A pooled filter workspace for the scope, acquired by the constructor: `rc` says whether there is one (check it before work()).
// Whatever is still on its stream has finished before the next call gets it.
struct FilterLease {
    wax_hip_engine* e;
    FilterWork* f = nullptr;
    const int rc;
    explicit FilterLease(wax_hip_engine* e_) : e(e_), rc(take_filter_work(e_, &f)) {}
    FilterLease(const FilterLease&) = delete;
    FilterWork& work() const { return *f; }
    ~FilterLease() { if (rc == WAX_HIP_OK) { (void)hipStreamSynchronize(f->stream); e->filter_works.release(f); } }
};

// room for m rows in the compact list (rows, their frame ids, their distances)
static int reserve_row_lists(FilterWork& f, uint64_t m) {
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

// A short allow-list, resolved on the host: allowed frame ids -> local rows, ascending and unique (row order is the tie-break order of
// every path), their ids beside them, both uploaded. With a predicate only the rows that pass it stay: the authoritative attribute
// columns are on the host too; with required terms (req) only the rows whose set holds them all. *m = rows staged; nothing is uploaded for 0.
static int stage_host_rows(wax_hip_engine* e, FilterWork& f, const uint64_t* allow, uint64_t n_allow, const wax_hip_row_predicate* pred, uint64_t* m,
                           const TermReq* req = nullptr) {
    std::vector<uint32_t> rows;
    rows.reserve((size_t)n_allow);
    for (uint64_t i = 0; i < n_allow; ++i) {
        const int64_t r = e->idmap.find(allow[i]);
        if (r < 0) continue;
        if (req && !term_row_has_all(e, (uint64_t)r, *req)) continue;   // the term column is authoritative on the host as well (DESIGN 4.11)
        if (!pred || predicate_passes(*pred, e->cols.ts().at((uint64_t)r), e->cols.flags().at((uint64_t)r))) rows.push_back((uint32_t)r);
    }
    std::sort(rows.begin(), rows.end());
    rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
    *m = rows.size();
    if (*m == 0) return WAX_HIP_OK;
    std::vector<uint64_t> ids(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) ids[i] = e->ids[rows[i]];
    { const int grc = reserve_row_lists(f, *m); if (grc != WAX_HIP_OK) return grc; }
    // pageable sources: the runtime stages them before returning, so the vectors may die at the end of this function
    HIP_TRY(hipMemcpyAsync(f.d_rows, rows.data(), rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, f.stream), WAX_HIP_ERR_INTERNAL, "row list upload");
    HIP_TRY(hipMemcpyAsync(f.d_ids, ids.data(), ids.size() * sizeof(uint64_t), hipMemcpyHostToDevice, f.stream), WAX_HIP_ERR_INTERNAL, "id list upload");
    HIP_TRY(hipStreamSynchronize(f.stream), WAX_HIP_ERR_INTERNAL, "row list upload");
    return WAX_HIP_OK;
}

// The gather tail: f.d_rows / f.d_ids hold the m passing rows ascending. Exact f32 distances with scan_kernel's lane mapping and
// summation order, the general selection, the hits on the host. `sync_what` names the search in the message of a device-side failure.
static int gather_topk(wax_hip_engine* e, FilterWork& f, const float* query, uint32_t dims, uint64_t m, int kpad, uint64_t* out_ids,
                       float* out_scores, uint32_t out_capacity, uint32_t* out_n, const char* sync_what) {
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
    HIP_TRY(launch_select_general(f.d_dist, (uint32_t)m, 0u, k_eff, k_eff, f.d_ids, f.sw, f.d_hits, st, nullptr, (int)e->select_grid.load()), WAX_HIP_ERR_INTERNAL, "select kernel launch");
    HIP_TRY(hipMemcpyAsync(f.h_hits, f.d_hits, (size_t)k_eff * sizeof(wax_hip_hit), hipMemcpyDeviceToHost, st), WAX_HIP_ERR_INTERNAL, "hits download");
    HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, sync_what);
    const int rc = hits_to_results(e->metric, f.h_hits, (uint32_t)k_eff, out_ids, out_scores, out_capacity, out_n);
    if (rc != WAX_HIP_OK) return rc;
    e->st_searches++;
    e->st_rows += m;
    e->st_bytes += m * (uint64_t)e->dims * 4ull;
    return WAX_HIP_OK;
}

// the per-workgroup key lists of either masked scan (+ the short merge's flag words, zero from the start)
static int reserve_partials(FilterWork& f) {
    if (f.d_partials) return WAX_HIP_OK;
    HIP_TRY(hipMalloc(&f.d_partials, kPartialsBytes), WAX_HIP_ERR_ALLOC, "Failed to allocate top-k stage buffer");
    HIP_TRY(hipMemsetAsync(partials_ticket(f.d_partials), 0, 128, f.stream), WAX_HIP_ERR_INTERNAL, "top-k stage buffer");
    return WAX_HIP_OK;
}

// The masked-scan tail: f.d_bitmap marks the m passing rows, live_chunks of the scan's chunks hold one. The f32 scan's rows, loads and
// arithmetic; chunks without a passing row are not read; the per-workgroup lists go through the second-launch merge.
static int masked_scan_topk(wax_hip_engine* e, FilterWork& f, const float* query, uint32_t dims, uint64_t m, uint64_t live_chunks, int kpad,
                            uint64_t* out_ids, float* out_scores, uint32_t out_capacity, uint32_t* out_n, const char* sync_what) {
    hipStream_t st = f.stream;
    const uint32_t count = (uint32_t)e->count, chunk_rows = scan_masked_chunk_rows(dims);
    { const int prc = reserve_partials(f); if (prc != WAX_HIP_OK) return prc; }
    const int k_eff = (uint64_t)kpad < m ? kpad : (int)m;
    const int cap = wave_list_cap(k_eff);
    HIP_TRY(hipMemcpyAsync(f.d_query, query, (size_t)dims * sizeof(float), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "query upload");
    MaskedScanArgs a{};
    a.store = e->d_store; a.query = f.d_query; a.bitmap = f.d_bitmap; a.partials = f.d_partials;
    a.n_rows = count; a.row_base = (uint32_t)e->row_base; a.dims = dims; a.k = k_eff; a.q_norm = query_norm(query, dims);
    int grid = 0;
    HIP_TRY(launch_scan_masked(a, e->metric, cap, (int)e->grid_blocks.load(), st, &grid), WAX_HIP_ERR_INTERNAL, "masked scan launch");
    { const int mrc = enqueue_list_merge(e, f.d_partials, grid, k_eff, k_eff, cap, a.row_base, a.n_rows, f.d_hits, st, nullptr); if (mrc != WAX_HIP_OK) return mrc; }
    HIP_TRY(hipMemcpyAsync(f.h_hits, f.d_hits, (size_t)k_eff * sizeof(wax_hip_hit), hipMemcpyDeviceToHost, st), WAX_HIP_ERR_INTERNAL, "hits download");
    HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, sync_what);
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

// May a predicate query for kpad results that the route rule sends to the masked scan stream the bf16 mirror ("predicate_mirror")?
// scan_uses_mirror's conditions (search_internal.inc) with this key in the place of "scan_mirror"; in auto mode "scan_mirror" 0
// switches this form off too. ("force_general" has already kept the query from the masked scan.)
static bool predicate_uses_mirror(wax_hip_engine* e, int kpad) {
    const int64_t mode = e->predicate_mirror.load();
    if (mode == 0 || kpad < 1 || kpad > MIRROR_MAX_K || !mirror_scan_supported(e->dims, e->metric)) return false;
    if (e->variant.load() > 0 || e->grid_blocks.load() > SCAN_KWAY_MERGE_GRID) return false;
    return mode >= 2 || (e->scan_mirror.load() != 0 && e->count * (uint64_t)e->dims * sizeof(float) > SCAN_KWAY_MAX_BYTES);
}

// The masked scan's mirror form (mirror_scan.hip; DESIGN 4.5): the bf16 mirror under the bitmap, the MIRROR_KP best approximate keys
// among the m > MIRROR_KP passing rows re-scored in f32, the answer released under the certificate — then it is the masked f32 scan's,
// bit for bit. live_mirror_chunks of the mirror kernel's chunks hold a passing row. Without a mirror, or without the certificate, the
// masked f32 scan answers on the same bitmap: no query fails because of the mirror.
static int masked_mirror_topk(wax_hip_engine* e, FilterWork& f, const float* query, uint32_t dims, uint64_t m, uint64_t live_chunks,
                              uint64_t live_mirror_chunks, int kpad, uint64_t* out_ids, float* out_scores, uint32_t out_capacity, uint32_t* out_n,
                              const char* sync_what) {
    hipStream_t st = f.stream;
    BatchMirror& b = e->batch;
    {
        const std::string keep = g_last_error;
        if (ensure_mirror(e, st) != WAX_HIP_OK || b.d_cb == nullptr || b.d_maxnorm == nullptr) {
            (void)hipGetLastError();                          // a refused allocation must not surface in the f32 launch behind it
            g_last_error = keep;
            e->st_predicate_mirror_unavailable++;
            return masked_scan_topk(e, f, query, dims, m, live_chunks, kpad, out_ids, out_scores, out_capacity, out_n, sync_what);
        }
    }
    { const int prc = reserve_partials(f); if (prc != WAX_HIP_OK) return prc; }
    constexpr size_t out_bytes = (size_t)(MIRROR_MAX_K + 1) * sizeof(wax_hip_hit);
    if (!f.d_mirror_out) HIP_TRY(hipMalloc(&f.d_mirror_out, out_bytes), WAX_HIP_ERR_ALLOC, "Failed to allocate mirror scan results");
    if (!f.h_mirror_out) HIP_TRY(hipHostMalloc(&f.h_mirror_out, out_bytes, hipHostMallocDefault), WAX_HIP_ERR_ALLOC, "Failed to allocate mirror scan results");
    const uint32_t count = (uint32_t)e->count, chunk_rows = mirror_masked_chunk_rows(dims);
    MirrorScanArgs a{};
    a.mirror = b.d_cb; a.store = e->d_store; a.partials = f.d_partials; a.ids = e->d_ids;
    a.hits = f.d_mirror_out; a.certified = reinterpret_cast<uint32_t*>(f.d_mirror_out + MIRROR_MAX_K); a.max_bits = b.d_maxnorm;
    a.n_rows = count; a.row_base = (uint32_t)e->row_base; a.dims = dims; a.k = kpad; a.kpad = kpad;   // (kpad <= MIRROR_MAX_K < m)
    a.q_norm = query_norm(query, dims);
    a.use_measured = e->batch_eps_measured.load() != 0 ? 1 : 0;
    HIP_TRY(launch_mirror_scan_masked(a, f.d_bitmap, query, e->metric, (int)e->grid_blocks.load(), st), WAX_HIP_ERR_INTERNAL, "masked mirror scan launch");
    HIP_TRY(hipMemcpyAsync(f.h_mirror_out, f.d_mirror_out, out_bytes, hipMemcpyDeviceToHost, st), WAX_HIP_ERR_INTERNAL, "hits download");
    HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, sync_what);
    const uint64_t n_chunks = ((uint64_t)count + chunk_rows - 1) / chunk_rows;
    e->st_predicate_skipped += n_chunks - live_mirror_chunks;
    e->st_rows += live_mirror_chunks * chunk_rows;
    e->st_bytes += live_mirror_chunks * chunk_rows * (uint64_t)dims * 2ull + (uint64_t)MIRROR_KP * dims * 4ull;
    if (*reinterpret_cast<const uint32_t*>(f.h_mirror_out + MIRROR_MAX_K) == 0u) {
        // the f32 route on the same bitmap: it counts the query (once) and adds its own figures
        e->st_predicate_mirror_fallbacks++;
        return masked_scan_topk(e, f, query, dims, m, live_chunks, kpad, out_ids, out_scores, out_capacity, out_n, sync_what);
    }
    const int rc = hits_to_results(e->metric, f.h_mirror_out, (uint32_t)kpad, out_ids, out_scores, out_capacity, out_n);
    if (rc != WAX_HIP_OK) return rc;
    e->st_searches++;
    e->st_predicate_masked++;
    e->st_predicate_mirror_scans++;
    return WAX_HIP_OK;
}

// ---- one query ----------------------------------------------------------------------

// One query with an allow-list (has_allow), a non-empty predicate (pred != nullptr) or both, on a pooled filter workspace; the caller
// holds the shared lock and has flushed pending rows. *out_n = results written (before any score cut). A list below
// "filter_device_min" is staged from the host; otherwise the passing rows are a device-side bitmap ([allow-list probe,] attribute
// mask), answered by gathering them or — predicate only — by the masked scan, over the f32 store or, on a large store, over the bf16
// mirror under the certificate ("predicate_mirror").
static int search_rows_locked(wax_hip_engine* e, const float* query, uint32_t dims, int kpad, int has_allow, const uint64_t* allow_frame_ids,
                              uint64_t n_allow, const wax_hip_row_predicate* user_pred, uint64_t* out_ids, float* out_scores,
                              uint32_t out_capacity, uint32_t* out_n, const TermReq* req) {
    *out_n = 0;
    // Required terms (wax_hip_search_terms; DESIGN 4.11) put term_mask_kernel in front of the attribute mask, which then always runs
    // — under a predicate that passes every row where the caller gave none — and stays the one place that counts.
    static const wax_hip_row_predicate pass_all{};
    const wax_hip_row_predicate* pred = user_pred ? user_pred : (req ? &pass_all : nullptr);
    if (req && e->cols.terms().empty()) { e->tm_host_decided++; return WAX_HIP_OK; }   // no frame has metadata: none matches (UnifiedSearch.swift:1219)
    if (pred) e->st_predicate_searches++;
    if (e->count == 0 || (has_allow && n_allow == 0)) return WAX_HIP_OK;
    if (pred && e->row_base + e->count > 0x100000000ull) return fail(WAX_HIP_ERR_CAPACITY, "row_base + count exceeds UInt32 row indices");
    FilterLease lease(e);
    if (lease.rc != WAX_HIP_OK) return lease.rc;
    FilterWork& f = lease.work();
    hipStream_t st = f.stream;
    const uint32_t count = (uint32_t)e->count;
    const char* sync_what = pred ? "predicate search failed on device" : "filtered search failed on device";
    const int64_t dev_min = e->filter_device_min.load();
    uint64_t m = 0;
    if (has_allow && !(dev_min >= 0 && n_allow >= (uint64_t)dev_min)) {
        { const int src = stage_host_rows(e, f, allow_frame_ids, n_allow, user_pred, &m, req); if (src != WAX_HIP_OK) return src; }
        if (req) e->tm_host_staged++;
        if (m == 0) return WAX_HIP_OK;
    } else {
        // ---- the row bitmap: [allow-list probe,] [attributes] ----
        // long lists: the probes are cache misses (~60 ns each on the host, 5.65 ms for 1M ids); on the device the same probes are a few
        // tens of microseconds against the id -> row table in HBM (filter.hip), and the bitmap they mark hands the rows back ascending
        // and unique
        const int64_t* d_ts = nullptr;
        const uint32_t* d_fl = nullptr;
        if (user_pred) { const int arc = ensure_attrs(e, st, &d_ts, &d_fl); if (arc != WAX_HIP_OK) return arc; }
        const uint32_t* d_term_off = nullptr;
        const uint32_t* d_term_val = nullptr;
        if (req) { const int trc = ensure_terms(e, st, &d_term_off, &d_term_val); if (trc != WAX_HIP_OK) return trc; }
        const uint64_t n_words = ((uint64_t)count + 31) / 32, n_blocks = filter_bitmap_blocks(count);
        int grc = grow_dev(&f.d_bitmap, &f.bitmap_words, n_words, sizeof(uint32_t), "Failed to allocate row bitmap");
        if (grc == WAX_HIP_OK) grc = grow_dev(&f.d_block_sum, &f.block_cap, n_blocks, sizeof(uint32_t), "Failed to allocate bitmap offsets");
        if (grc != WAX_HIP_OK) return grc;
        if (pred && !f.h_pred_counts)   // each word on its own test: a call that got one and was refused the other must not leave the next call a null pointer
            HIP_TRY(hipHostMalloc(&f.h_pred_counts, kPredCounts * sizeof(uint32_t), hipHostMallocDefault), WAX_HIP_ERR_ALLOC, "Failed to allocate predicate counters");
        if (pred && !f.d_pred_counts)
            HIP_TRY(hipMalloc(&f.d_pred_counts, kPredCounts * sizeof(uint32_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate predicate counters");
        if (has_allow) {
            // without a predicate the probe's launch also sums the bitmap (block offsets, total): the list is the whole filter
            { const int hrc = ensure_idhash(e, st); if (hrc != WAX_HIP_OK) return hrc; }
            grc = grow_dev(&f.d_allow, &f.allow_cap, n_allow, sizeof(uint64_t), "Failed to allocate allow-list");
            if (grc == WAX_HIP_OK && !pred) grc = reserve_row_lists(f, n_allow < e->count ? n_allow : e->count);
            if (grc != WAX_HIP_OK) return grc;
            HIP_TRY(hipMemcpyAsync(f.d_allow, allow_frame_ids, (size_t)n_allow * sizeof(uint64_t), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "allow-list upload");
            HIP_TRY(launch_allow_probe(f.d_allow, n_allow, e->d_ids, count, e->idhash.d_table, e->idhash.slots, f.d_bitmap,
                                       pred ? nullptr : f.d_block_sum, pred ? nullptr : f.d_total, st), WAX_HIP_ERR_INTERNAL, "allow-list probe launch");
            if (pred) e->st_filter_device++;
        }
        if (req) {
            // bit r = "row r holds every required term", ANDed into the probe's bitmap where there is a list; the attribute mask ANDs into it
            TermMaskArgs ta{};
            ta.off = d_term_off; ta.val = d_term_val; ta.bitmap = f.d_bitmap; ta.n_rows = count; ta.and_bitmap = has_allow ? 1 : 0;
            fill_term_mask_req(&ta, *req);
            HIP_TRY(launch_term_mask(ta, 0u, st), WAX_HIP_ERR_INTERNAL, "term mask launch");
            e->tm_device_masks++;
        }
        if (!pred) {
            HIP_TRY(launch_allow_emit(f.d_bitmap, count, f.d_block_sum, e->d_ids, f.d_rows, f.d_ids, st), WAX_HIP_ERR_INTERNAL, "allow-list compaction launch");
            HIP_TRY(hipMemcpyAsync(f.h_total, f.d_total, sizeof(uint32_t), hipMemcpyDeviceToHost, st), WAX_HIP_ERR_INTERNAL, "row count download");
            HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "allow-list probe failed on device");
            m = *f.h_total;
            e->st_filter_device++;   // (behind the synchronisation: a probe that failed on the device is not counted)
            if (m == 0) return WAX_HIP_OK;
        } else {
            const bool scan_shape = scan_masked_dims(dims) && kpad <= FUSED_MAX_K && e->force_general.load() == 0;   // kpad = clamp(top_k): top_k > 192 gathers
            const uint32_t chunk_rows = scan_shape ? scan_masked_chunk_rows(dims) : 0u;
            const uint32_t mirror_chunk_rows = scan_shape && predicate_uses_mirror(e, kpad) ? mirror_masked_chunk_rows(dims) : 0u;   // 0 = the mirror form is not taken
            AttrMaskArgs ma{};
            ma.ts = d_ts; ma.flags = d_fl; ma.bitmap = f.d_bitmap; ma.counts = f.d_pred_counts; ma.n_rows = count; ma.chunk_rows = chunk_rows; ma.chunk_rows2 = mirror_chunk_rows;
            ma.and_bitmap = (has_allow || req) ? 1 : 0;
            ma.has_after = pred->has_after != 0; ma.has_before = pred->has_before != 0; ma.after = pred->after; ma.before = pred->before; ma.deny_flags = pred->deny_flags;
            HIP_TRY(hipMemsetAsync(f.d_pred_counts, 0, kPredCounts * sizeof(uint32_t), st), WAX_HIP_ERR_INTERNAL, "predicate counters");
            HIP_TRY(launch_attr_mask(ma, st), WAX_HIP_ERR_INTERNAL, "attribute mask launch");
            HIP_TRY(hipMemcpyAsync(f.h_pred_counts, f.d_pred_counts, kPredCounts * sizeof(uint32_t), hipMemcpyDeviceToHost, st), WAX_HIP_ERR_INTERNAL, "row count download");
            HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "attribute mask failed on device");
            m = f.h_pred_counts[0];
            if (m == 0) return WAX_HIP_OK;
            // ---- route ----
            const int64_t route = e->predicate_route.load();
            if (scan_shape && route != 1 && (route == 2 || m * 1000ull >= (uint64_t)e->predicate_scan_min_permille.load() * (uint64_t)count)) {
                if (mirror_chunk_rows != 0u && m > (uint64_t)MIRROR_KP)   // with MIRROR_KP or fewer passing rows the finish cannot certify
                    return masked_mirror_topk(e, f, query, dims, m, f.h_pred_counts[1], f.h_pred_counts[2], kpad, out_ids, out_scores, out_capacity, out_n, sync_what);
                return masked_scan_topk(e, f, query, dims, m, f.h_pred_counts[1], kpad, out_ids, out_scores, out_capacity, out_n, sync_what);
            }
            { const int lrc = reserve_row_lists(f, m); if (lrc != WAX_HIP_OK) return lrc; }
            HIP_TRY(launch_bitmap_offsets(f.d_bitmap, count, f.d_block_sum, f.d_total, st), WAX_HIP_ERR_INTERNAL, "bitmap offsets launch");
            HIP_TRY(launch_allow_emit(f.d_bitmap, count, f.d_block_sum, e->d_ids, f.d_rows, f.d_ids, st), WAX_HIP_ERR_INTERNAL, "row compaction launch");
        }
    }
    const int rc = gather_topk(e, f, query, dims, m, kpad, out_ids, out_scores, out_capacity, out_n, sync_what);
    if (rc == WAX_HIP_OK && pred) e->st_predicate_gather++;
    return rc;
}

// wax_hip_search_filtered (pred == nullptr) and wax_hip_search_predicate (a non-empty predicate): argument checks, the sharded handle,
// then one device — the ordinary scan when there is neither list nor predicate, the locked body otherwise — and the score cut.
static int search_filtered_entry(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, int has_allow, const uint64_t* allow_frame_ids,
                                 uint64_t n_allow, int has_min_score, float min_score, const wax_hip_row_predicate* pred, uint64_t* out_ids,
                                 float* out_scores, uint32_t out_capacity, uint32_t* out_count) {
    if (out_count) *out_count = 0;
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (!query || !out_count || ((!out_ids || !out_scores) && out_capacity)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (has_allow && n_allow > 0 && !allow_frame_ids) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "allow-list is null");
    if (e->sh)
        return pred ? sh_search_predicate(e, query, dims, top_k, has_allow, allow_frame_ids, n_allow, has_min_score, min_score, pred, out_ids,
                                          out_scores, out_capacity, out_count)
                    : sh_search_filtered(e, query, dims, top_k, has_allow, allow_frame_ids, n_allow, has_min_score, min_score, out_ids,
                                         out_scores, out_capacity, out_count);
    if (dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));
    uint32_t n = 0;
    if (!has_allow && !pred) {
        // no allow-list: the ordinary scan, then the score cut
        const int rc = wax_hip_search(e, query, dims, top_k, out_ids, out_scores, out_capacity, &n);
        if (rc != WAX_HIP_OK) return rc;
    } else {
        DeviceGuard g(e->device);
        ReadGuard rd(e);
        { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return frc; }
        const int rc = search_rows_locked(e, query, dims, clamp_topk(top_k), has_allow, allow_frame_ids, n_allow, pred, out_ids, out_scores,
                                          out_capacity, &n);
        if (rc != WAX_HIP_OK) return rc;
    }
    if (has_min_score) apply_min_score(min_score, out_ids, out_scores, &n);
    *out_count = n;
    return WAX_HIP_OK;
}

int wax_hip_search_filtered(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, int has_allow,
                            const uint64_t* allow_frame_ids, uint64_t n_allow, int has_min_score, float min_score,
                            uint64_t* out_ids, float* out_scores, uint32_t out_capacity, uint32_t* out_count) {
    return search_filtered_entry(e, query, dims, top_k, has_allow, allow_frame_ids, n_allow, has_min_score, min_score, nullptr, out_ids, out_scores,
                                 out_capacity, out_count);
}

int wax_hip_search_predicate(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, int has_allow,
                             const uint64_t* allow_frame_ids, uint64_t n_allow, int has_min_score, float min_score,
                             const wax_hip_row_predicate* pred, uint64_t* out_ids, float* out_scores, uint32_t out_capacity,
                             uint32_t* out_count) {
    if (predicate_is_empty(pred))   // nothing to test per row: the filtered search (and, without a list, the ordinary scan) as it is
        return wax_hip_search_filtered(e, query, dims, top_k, has_allow, allow_frame_ids, n_allow, has_min_score, min_score, out_ids, out_scores,
                                       out_capacity, out_count);
    return search_filtered_entry(e, query, dims, top_k, has_allow, allow_frame_ids, n_allow, has_min_score, min_score, pred, out_ids, out_scores,
                                 out_capacity, out_count);
}

// ---- predicate tickets (DESIGN 4.5) -------------------------------------------

// wax_hip_search_predicate without an allow-list, as a ticket of wax_hip_search_collect. The routing is submit_impl's
// (api_search.inc): decided on the host where the store has no attributes, riding a masked pass over the code mirror where
// the rules of both ("predicate_mirror", "mirror_bits") and a free bitmap entry allow it, deferred to the blocking body otherwise.
int wax_hip_search_predicate_submit(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, int has_min_score, float min_score,
                                    const wax_hip_row_predicate* pred, uint64_t* out_ticket) {
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (!query || !out_ticket) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));
    const wax_hip_row_predicate np = normalised_predicate(pred);
    const TicketExtras x{has_min_score, min_score, predicate_is_empty(&np) ? nullptr : &np};   // empty: wax_hip_search_submit and the cut
    if (e->sh) return sh_submit(e, query, dims, top_k, out_ticket, &x);
    return submit_impl(e, query, dims, top_k, out_ticket, false, false, &x);
}

int wax_hip_predicate_ticket_stats(wax_hip_engine* e, wax_hip_predicate_ticket_stats_t* out) {
    if (!e || !out) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine/out is null");
    out->submitted = e->pt_submitted.load(); out->rode = e->pt_rode.load(); out->masked_passes = e->pt_masked_passes.load();
    out->certified = e->pt_certified.load(); out->fallbacks = e->pt_fallbacks.load(); out->deferred = e->pt_deferred.load();
    out->host_decided = e->pt_host_decided.load(); out->bitmap_builds = e->pt_bitmap_builds.load(); out->bitmap_hits = e->pt_bitmap_hits.load();
    return WAX_HIP_OK;
}

// ---- batched filtered search ------------------------------------------------

// The caller's arguments are sane for nq queries: both or neither of allow_begin / allow_len, every range inside the id array.
static int check_batch_allow(uint32_t nq, const uint64_t* allow, uint64_t n_allow_ids, const uint64_t* allow_begin, const uint64_t* allow_len) {
    if ((allow_begin == nullptr) != (allow_len == nullptr))
        return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "allow_begin and allow_len must both be given or both be null");
    if (!allow_len) return WAX_HIP_OK;
    for (uint32_t q = 0; q < nq; ++q) {
        const uint64_t len = allow_len[q];
        if (len == WAX_HIP_NO_ALLOW_LIST) continue;
        if (allow_begin[q] > n_allow_ids || len > n_allow_ids - allow_begin[q])
            return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "allow-list range of query " + std::to_string(q) + " leaves the id array");
        if (len > 0 && !allow) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "allow-list is null");
    }
    return WAX_HIP_OK;
}

// How the queries of one batched call are filtered: the caller's list arrays as they came (begin / len may be null: no query has a
// list) and the effective predicates (null: no query has one) — normalised, and empty where there is nothing to test per row.
struct BatchFilters {
    const uint64_t* allow;
    const uint64_t* begin;
    const uint64_t* len;
    const wax_hip_row_predicate* eff;
    bool listed(uint32_t q) const { return len != nullptr && len[q] != WAX_HIP_NO_ALLOW_LIST; }
    uint64_t length(uint32_t q) const { return listed(q) ? len[q] : 0; }
    const uint64_t* ids(uint32_t q) const { return length(q) ? allow + begin[q] : nullptr; }
    const wax_hip_row_predicate* pred(uint32_t q) const { return eff != nullptr && !predicate_is_empty(&eff[q]) ? &eff[q] : nullptr; }
};

// The queries with an allow-list, a predicate or both (fq), under the caller's shared lock: ONE gather pass for all of them. Queries
// with the same (list, predicate) share an ENTRY; every entry becomes a compact ascending row list with a device-side count
// (filter.hip sorts the short lists, a predicate's failures dropped before the sort; a long list takes the bitmap route, ANDed with
// the attribute mask; an entry without a list comes straight from the attribute columns, predicate.hip), multiscan.hip's gather form
// scores every row list against the queries that share it, the span merge attaches frame ids: one download, one synchronisation, no
// host round trip for a count. What that pass does not serve takes search_rows_locked per query.
// T (wax_hip_search_batch_terms; null: no query has a term set and nothing differs): a term set joins the entry's key. An entry
// without a list gets its set's row bitmap and passing count from term_mask_multi_kernel AHEAD of the layout — the one extra
// synchronisation — and its upper bound is that count; a short list's sort drops rows that lack a term; a long list with terms loops.
static int batch_filtered_locked(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int kpad, const std::vector<uint32_t>& fq,
                                 const BatchFilters& F, uint64_t n_allow_ids, const float* min_scores, uint64_t* out_ids, float* out_scores,
                                 uint32_t out_stride, uint32_t* out_counts, const BatchTerms* T = nullptr) {
    const uint64_t count = e->count;
    const int k = kpad < (int)out_stride ? kpad : (int)out_stride;   // the best out_stride of kpad: the same rows hits_to_results keeps
    const uint32_t group = (k >= 1 && k <= FUSED_MAX_K) ? scan_multi_group(dims, k) : 0u;
    auto term_req = [&](uint32_t q) -> const TermReq* { return T ? T->req(q) : nullptr; };   // (T: wax_hip_search_batch_terms, some query has a set)
    auto one = [&](uint32_t q) -> int {   // query q through the single-query body (which counts its own predicate search), then its cut
        uint32_t n = 0;
        const TermReq* req = term_req(q);
        if (req) { e->tm_searches++; e->tb_looped++; }   // wax_hip_search_terms' body: a looped term query counts itself as one of those
        const int rc = search_rows_locked(e, queries + (size_t)q * dims, dims, kpad, F.listed(q) ? 1 : 0, F.ids(q), F.length(q), F.pred(q),
                                          out_ids + (size_t)q * out_stride, out_scores + (size_t)q * out_stride, out_stride, &n, req);
        if (rc != WAX_HIP_OK) return rc;
        if (min_scores) apply_min_score(min_scores[q], out_ids + (size_t)q * out_stride, out_scores + (size_t)q * out_stride, &n);
        out_counts[q] = n;
        return WAX_HIP_OK;
    };
    if (e->filter_batch.load() == 0 || e->force_general.load() != 0 || group == 0) {
        for (uint32_t q : fq) { const int rc = one(q); if (rc != WAX_HIP_OK) return rc; }
        e->st_filter_batch_fallbacks += fq.size();
        return WAX_HIP_OK;
    }
    if (e->row_base + count > 0x100000000ull) return fail(WAX_HIP_ERR_CAPACITY, "row_base + count exceeds UInt32 row indices");
    // distinct entries: queries with the same (begin, len | no list, predicate, term set) share one. A term query without a predicate is
    // one whose predicate passes every row (DESIGN 4.11), so every term entry is an entry with a predicate below.
    static const wax_hip_row_predicate pass_all{};
    struct Entry {
        uint64_t begin, len, ub; uint32_t row_off; const wax_hip_row_predicate* pred; bool admitted; std::vector<uint32_t> qs;
        int32_t tset;    // its term set (T->sets), -1: none
        int32_t tslot;   // the bitmap of that set in f.d_tbits (entries without a list), -1: none
    };
    std::vector<Entry> lists;
    std::vector<uint8_t> apart(T ? nq : 0, 0);                    // term queries this pass does not answer: decided here, or looped
    uint64_t term_decided = 0;
    {
        typedef std::tuple<uint64_t, uint64_t, int32_t, int64_t, int32_t, int64_t, uint32_t, int32_t> EntryKey;
        std::map<EntryKey, uint32_t> index;
        for (uint32_t q : fq) {
            const int32_t ts = T ? T->of[q] : -1;
            if (ts >= 0 && e->cols.terms().empty()) { apart[q] = 1; ++term_decided; continue; }   // no frame has metadata: none matches (UnifiedSearch.swift:1219)
            const bool listed = F.listed(q);
            const uint64_t len = count == 0 ? 0 : (listed ? F.length(q) : WAX_HIP_NO_ALLOW_LIST);
            if (len == 0) continue;                               // nothing allowed: count 0
            const wax_hip_row_predicate* p = F.pred(q);
            if (ts >= 0 && !p) p = &pass_all;
            const uint64_t begin = listed ? F.begin[q] : 0;
            const EntryKey key = p ? EntryKey(begin, len, p->has_after, p->after, p->has_before, p->before, p->deny_flags, ts) : EntryKey(begin, len, 0, 0, 0, 0, 0u, ts);
            auto it = index.emplace(key, (uint32_t)lists.size());
            if (it.second) lists.push_back(Entry{begin, len, listed && len < count ? len : count, 0, p, true, {}, ts, -1});
            lists[it.first->second].qs.push_back(q);
        }
    }
    e->tb_host_decided += term_decided;
    std::vector<uint32_t> looped;
    // Term entries (wax_hip_search_batch_terms). One with a list too long for the LDS sort takes the single-query body. One without a list
    // gets its set's row bitmap from term_mask_multi_kernel: sets are admitted in order of their first query while there are at most
    // kTermBatchMaxSets of them and their bitmaps fit kTermBatchMaxBytes (a memory cap); the entries of the rest are looped.
    constexpr uint64_t kTermBatchMaxSets = 256, kTermBatchMaxBytes = 256ull << 20;
    std::vector<int32_t> slot_set;                                // bitmap slot -> term set
    const uint64_t tstride = term_multi_stride_words((uint32_t)count);
    if (T) {
        std::map<int32_t, int32_t> slot_of;
        for (Entry& L : lists) {
            if (L.tset < 0) continue;
            bool admit = true;
            if (L.len != WAX_HIP_NO_ALLOW_LIST) {
                admit = L.len <= ROWLIST_SORT_MAX;
            } else {
                auto it = slot_of.find(L.tset);
                if (it == slot_of.end()) {
                    admit = slot_set.size() < kTermBatchMaxSets && (slot_set.size() + 1) * tstride * sizeof(uint32_t) <= kTermBatchMaxBytes;
                    if (admit) { it = slot_of.emplace(L.tset, (int32_t)slot_set.size()).first; slot_set.push_back(L.tset); }
                }
                if (admit) L.tslot = it->second;
            }
            if (!admit) { L.admitted = false; looped.insert(looped.end(), L.qs.begin(), L.qs.end()); }
        }
    }
    // The term pass: the CSR column once per 32 admitted sets -> one bitmap and one passing count per set; the counts come to the host
    // (the one extra synchronisation, only in calls with such entries) and become the entries' upper bounds. A count of 0 ends an entry.
    // The workspace stays with the call from here on, so what is looped waits until the pass has given it back (see below).
    std::unique_ptr<FilterLease> lease;
    const uint32_t* d_term_off = nullptr;
    const uint32_t* d_term_val = nullptr;
    if (!slot_set.empty()) {
        lease.reset(new FilterLease(e));
        if (lease->rc != WAX_HIP_OK) return lease->rc;
        FilterWork& f = lease->work();
        hipStream_t st = f.stream;
        { const int trc = ensure_terms(e, st, &d_term_off, &d_term_val); if (trc != WAX_HIP_OK) return trc; }
        const uint32_t S = (uint32_t)slot_set.size(), n_launch = (S + TERM_MULTI_MAX_SETS - 1) / TERM_MULTI_MAX_SETS;
        const uint64_t table_words = 2ull * TERM_MULTI_MAX_UNION, cnt0 = (uint64_t)n_launch * table_words;
        int grc = grow_dev(&f.d_tplan, &f.tplan_cap, cnt0 + S, sizeof(uint32_t), "Failed to allocate term-set tables");
        if (grc == WAX_HIP_OK) grc = grow_dev(&f.d_tbits, &f.tbits_cap, (uint64_t)S * tstride, sizeof(uint32_t), "Failed to allocate term-set bitmaps");
        if (grc != WAX_HIP_OK) return grc;
        std::vector<uint32_t> tp((size_t)(cnt0 + S), 0u);         // per launch its tables, then the counts (zero)
        std::vector<TermMaskMultiArgs> targs(n_launch);
        for (uint32_t l = 0; l < n_launch; ++l) {
            const uint32_t s0 = l * TERM_MULTI_MAX_SETS, sn = std::min<uint32_t>(TERM_MULTI_MAX_SETS, S - s0);
            const TermReq* sets[TERM_MULTI_MAX_SETS];
            for (uint32_t s = 0; s < sn; ++s) sets[s] = &T->sets[(size_t)slot_set[s0 + s]];
            TermMultiPlan plan;
            make_term_multi_plan(sets, sn, &plan);
            std::memcpy(tp.data() + (size_t)l * table_words, plan.tables, sizeof(plan.tables));
            TermMaskMultiArgs& a = targs[l];
            a = TermMaskMultiArgs{};
            a.off = d_term_off; a.val = d_term_val; a.uni = f.d_tplan + (size_t)l * table_words; a.memb = a.uni + TERM_MULTI_MAX_UNION;
            a.bitmaps = f.d_tbits + (size_t)s0 * tstride; a.counts = f.d_tplan + cnt0 + s0;
            a.n_rows = (uint32_t)count; a.n_union = plan.n_union; a.n_sets = sn; a.stride_words = (uint32_t)tstride;
            for (int b = 0; b < 5; ++b) a.nbits[b] = plan.nbits[b];
        }
        HIP_TRY(hipMemcpyAsync(f.d_tplan, tp.data(), tp.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "term-set table upload");
        for (uint32_t l = 0; l < n_launch; ++l) HIP_TRY(launch_term_mask_multi(targs[l], 0u, st), WAX_HIP_ERR_INTERNAL, "term mask launch");
        std::vector<uint32_t> tcnt(S);
        HIP_TRY(hipMemcpyAsync(tcnt.data(), f.d_tplan + cnt0, (size_t)S * sizeof(uint32_t), hipMemcpyDeviceToHost, st), WAX_HIP_ERR_INTERNAL, "term count download");
        HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "term mask failed on device");
        e->tb_mask_launches += n_launch;
        for (Entry& L : lists)
            if (L.tslot >= 0) { L.ub = tcnt[(size_t)L.tslot]; if (L.ub == 0) L.admitted = false; }
    }
    // the row-slot budget of the entries with a predicate, in order of their first query (an entry without a list costs `count` slots
    // whatever passes — or, with a term set, the rows that hold the set); what does not fit takes the single-query body below
    uint64_t pred_entries = 0, attr_entries = 0;
    bool short_terms = false;
    {
        const uint64_t budget = (uint64_t)e->predicate_batch_rows.load();
        uint64_t used = 0;
        for (Entry& L : lists) {
            if (!L.pred || !L.admitted) continue;
            if (L.ub <= budget - used) {
                used += L.ub; ++pred_entries;
                attr_entries += predicate_is_empty(L.pred) ? 0u : 1u;
                short_terms = short_terms || (L.tset >= 0 && L.tslot < 0);
                continue;
            }
            L.admitted = false;
            looped.insert(looped.end(), L.qs.begin(), L.qs.end());
        }
    }
    for (uint32_t q : looped) if (T) apart[q] = 1;
    if (T) {
        std::vector<uint8_t> sent(T->sets.size(), 0);
        uint64_t n_sent = 0, n_answered = 0;
        for (int32_t s : slot_set) if (!sent[(size_t)s]) { sent[(size_t)s] = 1; ++n_sent; }
        for (const Entry& L : lists)
            if (L.admitted && L.tset >= 0 && !sent[(size_t)L.tset]) { sent[(size_t)L.tset] = 1; ++n_sent; }
        for (uint32_t q : fq) n_answered += (T->of[q] >= 0 && !apart[q]) ? 1u : 0u;
        e->tb_sets += n_sent;
        e->tb_queries += n_answered;
    }
    uint64_t rows_total = 0, long_max = 0, attr_items = 0;
    uint32_t short_max = 0, short_max_pred = 0;
    bool any_listed = false;
    std::vector<RowListDesc> descs, descs_pred;
    std::vector<RowListPred> sort_preds;
    std::vector<AttrRowsRecord> records;
    std::vector<uint32_t> item_rec;
    const uint32_t long_blocks = filter_bitmap_blocks((uint32_t)count);   // the bitmap route's share of d_block_sum; the records' slots follow it
    auto pred_fields = [](const wax_hip_row_predicate& p, auto& out) {
        out.has_after = p.has_after; out.has_before = p.has_before; out.after = p.after; out.before = p.before; out.deny_flags = p.deny_flags;
    };
    for (uint32_t li = 0; li < lists.size(); ++li) {
        Entry& L = lists[li];
        if (!L.admitted) continue;
        L.row_off = (uint32_t)rows_total;
        rows_total += L.ub;
        if (rows_total >= 0x80000000ull) return fail(WAX_HIP_ERR_CAPACITY, "allowed rows of one batch exceed 2^31");
        if (L.len == WAX_HIP_NO_ALLOW_LIST) {
            AttrRowsRecord r{};
            r.n_rows = (uint32_t)count; r.row_off = L.row_off; r.count_slot = li;
            r.n_items = (uint32_t)((count + ATTR_ROWS_ITEM - 1) / ATTR_ROWS_ITEM); r.item0 = (uint32_t)attr_items; r.block0 = long_blocks + (uint32_t)attr_items;
            pred_fields(*L.pred, r);
            if (L.tslot >= 0) r.bitmap = lease->work().d_tbits + (size_t)L.tslot * tstride;   // its set's rows: at most ub of them pass
            for (uint32_t i = 0; i < r.n_items; ++i) item_rec.push_back((uint32_t)records.size());
            attr_items += r.n_items;
            if (attr_items >= 0x80000000ull) return fail(WAX_HIP_ERR_CAPACITY, "too many work items in one batch");
            records.push_back(r);
            continue;
        }
        any_listed = true;
        if (L.len > ROWLIST_SORT_MAX) {
            if (L.ub > long_max) long_max = L.ub;
        } else if (L.pred) {
            RowListPred sp{};
            pred_fields(*L.pred, sp);
            if (L.tset >= 0) {   // the sort drops a probed row that lacks a required term (the column's pointers follow below)
                const TermReq& req = T->sets[(size_t)L.tset];
                sp.n_terms = req.n;
                for (int i = 0; i < TERMS_MAX_REQUIRED; ++i) sp.terms[i] = req.t[(uint32_t)i < req.n ? i : 0];
            }
            sort_preds.push_back(sp);
            descs_pred.push_back(RowListDesc{L.begin, (uint32_t)L.len, L.row_off, li, 0u});
            if (L.len > short_max_pred) short_max_pred = (uint32_t)L.len;
        } else {
            descs.push_back(RowListDesc{L.begin, (uint32_t)L.len, L.row_off, li, 0u});
            if (L.len > short_max) short_max = (uint32_t)L.len;
        }
    }
    // groups of up to `group` queries per entry, work items sized by the entry's upper bound (its device-side length is not read back)
    std::vector<GatherGroup> groups;
    std::vector<uint32_t> item_group, slot_q, spans;
    std::vector<float> slot_norm;
    uint64_t part_lists = 0;
    const int grid_cap = (int)e->grid_blocks.load();
    for (uint32_t li = 0; li < lists.size(); ++li) {
        const Entry& L = lists[li];
        if (!L.admitted) continue;
        const uint32_t W = scan_multi_listed_items(L.ub, dims, grid_cap);
        for (size_t g0 = 0; g0 < L.qs.size(); g0 += group) {
            const uint32_t gn = (uint32_t)std::min<size_t>(group, L.qs.size() - g0);
            GatherGroup G{};
            G.row_off = L.row_off; G.count_slot = li; G.q0 = (uint32_t)slot_q.size(); G.nq = gn;
            G.part_off = (uint32_t)part_lists; G.n_items = W; G.item0 = (uint32_t)item_group.size();
            for (uint32_t i = 0; i < gn; ++i) {
                const uint32_t q = L.qs[g0 + i];
                slot_q.push_back(q);
                slot_norm.push_back(query_norm(queries + (size_t)q * dims, dims));
                spans.push_back((uint32_t)(part_lists + (uint64_t)i * W));
                spans.push_back(W);
            }
            for (uint32_t w = 0; w < W; ++w) item_group.push_back((uint32_t)groups.size());
            groups.push_back(G);
            part_lists += (uint64_t)gn * W;
            if (part_lists >= 0x80000000ull / (uint64_t)k) return fail(WAX_HIP_ERR_CAPACITY, "too many partial lists in one batch");
        }
    }
    for (uint32_t q : fq) out_counts[q] = 0;
    const uint32_t P = (uint32_t)slot_q.size();
    const uint64_t passed = fq.size() - looped.size() - term_decided;
    e->st_filter_batch_queries += passed;
    e->st_searches += passed;
    if (F.eff || T) {
        // the predicates this pass answers (one without a row to offer included; a term query counts as one, DESIGN 4.11); a looped query
        // is counted by the single-query body
        std::vector<uint8_t> is_looped(nq, 0);
        for (uint32_t q : looped) is_looped[q] = 1;
        uint64_t n = 0;
        for (uint32_t q : fq) n += ((F.pred(q) != nullptr || (term_req(q) != nullptr && !apart[q])) && !is_looped[q]) ? 1u : 0u;
        e->st_predicate_searches += n;
        e->st_predicate_batch_queries += n;
        e->st_predicate_batch_classes += pred_entries;
    }
    // The looped queries go ahead of the pass and of its workspace: the single-query body leases a workspace of its own, and a call that
    // held one while it waited for another could wait for a call doing the same. A call whose term pass already holds the workspace
    // loops them behind the pass instead, once the workspace is given back.
    const bool loop_first = lease == nullptr;
    auto run_looped = [&]() -> int {
        for (uint32_t q : looped) { const int rc = one(q); if (rc != WAX_HIP_OK) return rc; }
        e->st_filter_batch_fallbacks += looped.size();
        return WAX_HIP_OK;
    };
    if (loop_first) { const int lrc = run_looped(); if (lrc != WAX_HIP_OK) return lrc; }
    auto pass = [&]() -> int {
    if (!lease) lease.reset(new FilterLease(e));
    if (lease->rc != WAX_HIP_OK) return lease->rc;
    FilterWork& f = lease->work();
    hipStream_t st = f.stream;
    if (any_listed) { const int hrc = ensure_idhash(e, st); if (hrc != WAX_HIP_OK) return hrc; }
    const int64_t* d_ts = nullptr;
    const uint32_t* d_fl = nullptr;
    if (attr_entries != 0) {
        // the attribute columns, once, on this stream under the lock held (null: a store without attributes reads (0, 0) in every row);
        // an entry whose predicate passes every row (a term query without one) does not read them
        { const int arc = ensure_attrs(e, st, &d_ts, &d_fl); if (arc != WAX_HIP_OK) return arc; }
        for (AttrRowsRecord& r : records)
            if (r.has_after != 0 || r.has_before != 0 || r.deny_flags != 0u) { r.ts = d_ts; r.flags = d_fl; }
        for (RowListPred& sp : sort_preds)
            if (sp.has_after != 0 || sp.has_before != 0 || sp.deny_flags != 0u) { sp.ts = d_ts; sp.flags = d_fl; }
        if (long_max > 0 && !f.d_pred_counts)
            HIP_TRY(hipMalloc(&f.d_pred_counts, kPredCounts * sizeof(uint32_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate predicate counters");
    }
    if (short_terms) {
        // the term column for the sorted lists' term test (ensure_terms is the only uploader; the term pass above has called it already)
        if (!d_term_off) { const int trc = ensure_terms(e, st, &d_term_off, &d_term_val); if (trc != WAX_HIP_OK) return trc; }
        for (RowListPred& sp : sort_preds) { sp.term_off = d_term_off; sp.term_val = d_term_val; }
    }
    // one blob: descs | descs with a predicate | their predicates | attribute records | their work table | groups | item_group | slot_q |
    // slot_norm | spans (16-byte aligned sections)
    auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t o_desc = 0, o_dpred = al(o_desc + descs.size() * sizeof(RowListDesc)), o_spred = al(o_dpred + descs_pred.size() * sizeof(RowListDesc));
    const size_t o_rec = al(o_spred + sort_preds.size() * sizeof(RowListPred)), o_irec = al(o_rec + records.size() * sizeof(AttrRowsRecord));
    const size_t o_grp = al(o_irec + item_rec.size() * 4), o_item = al(o_grp + groups.size() * sizeof(GatherGroup));
    const size_t o_q = al(o_item + item_group.size() * 4), o_n = al(o_q + (size_t)P * 4), o_sp = al(o_n + (size_t)P * 4), meta_bytes = al(o_sp + (size_t)P * 8);
    std::vector<unsigned char> meta(meta_bytes, 0);
    std::memcpy(meta.data() + o_desc, descs.data(), descs.size() * sizeof(RowListDesc));
    std::memcpy(meta.data() + o_dpred, descs_pred.data(), descs_pred.size() * sizeof(RowListDesc));
    std::memcpy(meta.data() + o_spred, sort_preds.data(), sort_preds.size() * sizeof(RowListPred));
    std::memcpy(meta.data() + o_rec, records.data(), records.size() * sizeof(AttrRowsRecord));
    std::memcpy(meta.data() + o_irec, item_rec.data(), item_rec.size() * 4);
    std::memcpy(meta.data() + o_grp, groups.data(), groups.size() * sizeof(GatherGroup));
    std::memcpy(meta.data() + o_item, item_group.data(), item_group.size() * 4);
    std::memcpy(meta.data() + o_q, slot_q.data(), (size_t)P * 4);
    std::memcpy(meta.data() + o_n, slot_norm.data(), (size_t)P * 4);
    std::memcpy(meta.data() + o_sp, spans.data(), (size_t)P * 8);
    int grc = grow_dev(&f.d_meta, &f.meta_cap, meta_bytes, 1, "Failed to allocate batch filter tables");
    if (grc == WAX_HIP_OK) grc = grow_dev(&f.d_allow, &f.allow_cap, n_allow_ids, sizeof(uint64_t), "Failed to allocate allow-lists");
    if (grc == WAX_HIP_OK) grc = grow_dev(&f.d_bq, &f.bq_cap, (uint64_t)nq * dims, sizeof(float), "Failed to allocate batch queries");
    if (grc == WAX_HIP_OK) grc = grow_dev(&f.d_lrows, &f.lrows_cap, rows_total, sizeof(uint32_t), "Failed to allocate allowed-row lists");
    if (grc == WAX_HIP_OK) grc = grow_dev(&f.d_lcnt, &f.lcnt_cap, lists.size(), sizeof(uint32_t), "Failed to allocate allowed-row counts");
    if (grc == WAX_HIP_OK) grc = grow_dev(&f.d_part, &f.part_cap, part_lists * (uint64_t)k, sizeof(int64_t), "Failed to allocate gather partials");
    if (grc == WAX_HIP_OK) grc = grow_dev(&f.d_bhits, &f.bhits_cap, (uint64_t)P * k, sizeof(wax_hip_hit), "Failed to allocate batch filter hits");
    if (grc == WAX_HIP_OK && long_max > 0) {
        const uint64_t n_words = (count + 31) / 32;
        grc = grow_dev(&f.d_bitmap, &f.bitmap_words, n_words, sizeof(uint32_t), "Failed to allocate row bitmap");
        if (grc == WAX_HIP_OK) grc = grow_dev(&f.d_lids, &f.lids_cap, long_max, sizeof(uint64_t), "Failed to allocate allowed-id list");
    }
    if (grc == WAX_HIP_OK && (long_max > 0 || attr_items > 0))
        grc = grow_dev(&f.d_block_sum, &f.block_cap, (uint64_t)long_blocks + attr_items, sizeof(uint32_t), "Failed to allocate bitmap offsets");
    if (grc != WAX_HIP_OK) return grc;
    const RowListDesc* d_desc = reinterpret_cast<const RowListDesc*>(f.d_meta + o_desc);
    const RowListDesc* d_desc_pred = reinterpret_cast<const RowListDesc*>(f.d_meta + o_dpred);
    const RowListPred* d_sort_preds = reinterpret_cast<const RowListPred*>(f.d_meta + o_spred);
    const AttrRowsRecord* d_rec = reinterpret_cast<const AttrRowsRecord*>(f.d_meta + o_rec);
    const uint32_t* d_item_rec = reinterpret_cast<const uint32_t*>(f.d_meta + o_irec);
    const GatherGroup* d_grp = reinterpret_cast<const GatherGroup*>(f.d_meta + o_grp);
    const uint32_t* d_item = reinterpret_cast<const uint32_t*>(f.d_meta + o_item);
    const uint32_t* d_slot_q = reinterpret_cast<const uint32_t*>(f.d_meta + o_q);
    const float* d_slot_n = reinterpret_cast<const float*>(f.d_meta + o_n);
    const uint32_t* d_spans = reinterpret_cast<const uint32_t*>(f.d_meta + o_sp);
    // the caller's id array as it is (the lists are ranges of it; overlapping ranges travel once), the queries, the tables
    HIP_TRY(hipMemcpyAsync(f.d_allow, F.allow, (size_t)n_allow_ids * sizeof(uint64_t), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "allow-list upload");
    HIP_TRY(hipMemcpyAsync(f.d_bq, queries, (size_t)nq * dims * sizeof(float), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "query upload");
    HIP_TRY(hipMemcpyAsync(f.d_meta, meta.data(), meta_bytes, hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "batch filter table upload");
    // entries -> compact ascending row lists with device-side counts; no host round trip before the scan
    HIP_TRY(launch_rowlist_sort(f.d_allow, d_desc, nullptr, (uint32_t)descs.size(), short_max, e->d_ids, e->idhash.d_table, e->idhash.slots, f.d_lrows,
                                f.d_lcnt, st), WAX_HIP_ERR_INTERNAL, "allow-list sort launch");
    HIP_TRY(launch_rowlist_sort(f.d_allow, d_desc_pred, d_sort_preds, (uint32_t)descs_pred.size(), short_max_pred, e->d_ids, e->idhash.d_table,
                                e->idhash.slots, f.d_lrows, f.d_lcnt, st), WAX_HIP_ERR_INTERNAL, "allow-list sort launch");
    if (!records.empty())   // every entry without a list, straight from the attribute columns: three launches whatever their number
        HIP_TRY(launch_attr_rows(d_rec, (uint32_t)records.size(), d_item_rec, (uint32_t)item_rec.size(), f.d_block_sum, f.d_lrows, f.d_lcnt, st),
                WAX_HIP_ERR_INTERNAL, "attribute row-list launch");
    for (uint32_t li = 0; li < lists.size(); ++li) {   // lists too long for LDS: the single-query path's bitmap route, one list at a time
        const Entry& L = lists[li];
        if (!L.admitted || L.len == WAX_HIP_NO_ALLOW_LIST || L.len <= ROWLIST_SORT_MAX) continue;
        HIP_TRY(launch_allow_probe(f.d_allow + L.begin, L.len, e->d_ids, (uint32_t)count, e->idhash.d_table, e->idhash.slots, f.d_bitmap,
                                   L.pred ? nullptr : f.d_block_sum, L.pred ? nullptr : f.d_lcnt + li, st), WAX_HIP_ERR_INTERNAL, "allow-list probe launch");
        if (L.pred) {
            AttrMaskArgs ma{};
            ma.ts = d_ts; ma.flags = d_fl;
            ma.bitmap = f.d_bitmap; ma.counts = f.d_pred_counts; ma.n_rows = (uint32_t)count; ma.chunk_rows = 0; ma.and_bitmap = 1;
            pred_fields(*L.pred, ma);
            HIP_TRY(hipMemsetAsync(f.d_pred_counts, 0, kPredCounts * sizeof(uint32_t), st), WAX_HIP_ERR_INTERNAL, "predicate counters");
            HIP_TRY(launch_attr_mask(ma, st), WAX_HIP_ERR_INTERNAL, "attribute mask launch");
            HIP_TRY(launch_bitmap_offsets(f.d_bitmap, (uint32_t)count, f.d_block_sum, f.d_lcnt + li, st), WAX_HIP_ERR_INTERNAL, "bitmap offsets launch");
        }
        HIP_TRY(launch_allow_emit(f.d_bitmap, (uint32_t)count, f.d_block_sum, e->d_ids, f.d_lrows + L.row_off, f.d_lids, st),
                WAX_HIP_ERR_INTERNAL, "allow-list compaction launch");
        e->st_filter_device++;
    }
    ScanMultiArgs a{};
    a.store = e->d_store; a.queries = f.d_bq; a.qlist = d_slot_q; a.q_norm = d_slot_n; a.partials = f.d_part;
    a.n_rows = (uint32_t)count; a.row_base = (uint32_t)e->row_base; a.dims = dims; a.nq = 0; a.k = k;
    a.rows = f.d_lrows; a.row_counts = f.d_lcnt; a.groups = d_grp; a.item_group = d_item;
    HIP_TRY(launch_scan_multi_listed(a, e->metric, (uint32_t)item_group.size(), st), WAX_HIP_ERR_INTERNAL, "gather scan launch");
    HIP_TRY(launch_merge_keys_spans(f.d_part, d_spans, k, e->d_ids, a.row_base, (uint32_t)count, f.d_bhits, (uint32_t)k, P, st),
            WAX_HIP_ERR_INTERNAL, "gather merge launch");
    std::vector<wax_hip_hit> hits((size_t)P * k);
    std::vector<uint32_t> lcnt(pred_entries != 0 ? lists.size() : 0);   // what the entries with a predicate passed: for the accounting only
    HIP_TRY(hipMemcpyAsync(hits.data(), f.d_bhits, hits.size() * sizeof(wax_hip_hit), hipMemcpyDeviceToHost, st), WAX_HIP_ERR_INTERNAL, "hits download");
    if (!lcnt.empty())
        HIP_TRY(hipMemcpyAsync(lcnt.data(), f.d_lcnt, lcnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st), WAX_HIP_ERR_INTERNAL, "row count download");
    HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "batched filtered search failed on device");
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t q = slot_q[p];
        uint32_t n = 0;
        hits_to_results(e->metric, hits.data() + (size_t)p * k, (uint32_t)k, out_ids + (size_t)q * out_stride, out_scores + (size_t)q * out_stride,
                        out_stride, &n);
        if (min_scores) apply_min_score(min_scores[q], out_ids + (size_t)q * out_stride, out_scores + (size_t)q * out_stride, &n);
        out_counts[q] = n;
    }
    // an entry without a predicate is charged its upper bound, one with a predicate the rows it passed
    uint64_t rows_read = 0;
    for (uint32_t li = 0; li < lists.size(); ++li)
        if (lists[li].admitted) rows_read += lists[li].pred ? (uint64_t)lcnt[li] : lists[li].ub;
    e->st_rows += rows_read;
    e->st_bytes += rows_read * (uint64_t)dims * 4ull;
    return WAX_HIP_OK;
    };
    const int prc = P == 0 ? WAX_HIP_OK : pass();
    lease.reset();                                             // (waits for what is still on the workspace's stream)
    if (prc != WAX_HIP_OK) return prc;
    return loop_first ? WAX_HIP_OK : run_looped();
}

// wax_hip_search_batch_predicate and wax_hip_search_batch_terms: one body. term_begin / term_len null: no query has a term set, and
// nothing below differs from the call as it was before the term arguments existed.
static int search_batch_rows_entry(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k,
                                   const uint64_t* allow_frame_ids, uint64_t n_allow_ids, const uint64_t* allow_begin,
                                   const uint64_t* allow_len, const float* min_scores, const wax_hip_row_predicate* preds,
                                   const uint32_t* required_terms, uint64_t n_required_terms, const uint64_t* term_begin,
                                   const uint32_t* term_len, uint64_t* out_ids, float* out_scores, uint32_t out_stride, uint32_t* out_counts) {
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (nq == 0) return WAX_HIP_OK;
    if (!queries || !out_counts) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null input");
    if ((!out_ids || !out_scores) && out_stride) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "output arrays are null");
    { const int crc = check_batch_allow(nq, allow_frame_ids, n_allow_ids, allow_begin, allow_len); if (crc != WAX_HIP_OK) return crc; }
    // every refusal precedes the first write to the outputs: the dimension check (the call's own, the handle's and the shards' alike) too
    if ((term_begin || term_len) && dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));
    BatchTerms terms;
    bool any_terms = false;
    { const int trc = make_batch_terms(nq, required_terms, n_required_terms, term_begin, term_len, &terms, &any_terms); if (trc != WAX_HIP_OK) return trc; }
    for (uint32_t q = 0; q < nq; ++q) out_counts[q] = 0;
    if (e->sh) return sh_search_batch_predicate(e, queries, nq, dims, top_k, allow_frame_ids, n_allow_ids, allow_begin, allow_len, min_scores, preds,
                                                out_ids, out_scores, out_stride, out_counts, required_terms, n_required_terms,
                                                any_terms ? term_begin : nullptr, any_terms ? term_len : nullptr);
    if (dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));
    if (out_stride == 0) return WAX_HIP_OK;
    const BatchTerms* T = any_terms ? &terms : nullptr;
    if (T) e->tb_calls++;
    // The effective predicates: normalised, and — on a store that never had attributes, where every row reads (0, 0) — decided here,
    // once for all rows: the query loses its predicate, or its count stays 0 without device work (`dead`).
    std::vector<wax_hip_row_predicate> eff;
    std::vector<uint8_t> dead;
    bool any_pred = false;
    for (uint32_t q = 0; preds && q < nq && !any_pred; ++q) any_pred = !predicate_is_empty(&preds[q]);
    if (any_pred) {
        bool has_attrs;
        { ReadGuard rd(e); has_attrs = e->cols.has_attributes(); }
        eff.resize(nq);
        dead.assign(nq, 0);
        for (uint32_t q = 0; q < nq; ++q) {
            wax_hip_row_predicate np = normalised_predicate(&preds[q]);
            if (!predicate_is_empty(&np) && !has_attrs) {
                if (predicate_passes(np, 0, 0u)) np = wax_hip_row_predicate{};
                else dead[q] = 1;
            }
            eff[q] = np;
        }
    }
    const BatchFilters F{allow_frame_ids, allow_begin, allow_len, any_pred ? eff.data() : nullptr};
    std::vector<uint32_t> plain, fq;
    for (uint32_t q = 0; q < nq; ++q) {
        if (any_pred && dead[q]) continue;
        (F.listed(q) || F.pred(q) || (T && T->of[q] >= 0) ? fq : plain).push_back(q);
    }
    if (!plain.empty()) {
        // queries with neither list nor predicate: one sub-batch of the unfiltered batched search (its own lock acquisition), then the cut
        std::vector<float> qs;
        const float* src = queries;
        if (plain.size() != nq) {
            qs.resize(plain.size() * (size_t)dims);
            for (size_t i = 0; i < plain.size(); ++i) std::memcpy(qs.data() + i * dims, queries + (size_t)plain[i] * dims, (size_t)dims * 4);
            src = qs.data();
        }
        const uint32_t limit = (uint32_t)clamp_topk(top_k);
        const uint32_t w = limit < out_stride ? limit : out_stride;
        std::vector<wax_hip_hit> hits(plain.size() * (size_t)w);
        std::vector<uint32_t> cnt(plain.size(), 0);
        const int rc = search_batch_hits_impl(e, src, (uint32_t)plain.size(), dims, top_k, hits.data(), w, cnt.data());
        if (rc != WAX_HIP_OK) return rc;
        for (size_t i = 0; i < plain.size(); ++i) {
            const uint32_t q = plain[i];
            uint32_t n = 0;
            hits_to_results(e->metric, hits.data() + i * w, w, out_ids + (size_t)q * out_stride, out_scores + (size_t)q * out_stride, out_stride, &n);
            if (min_scores) apply_min_score(min_scores[q], out_ids + (size_t)q * out_stride, out_scores + (size_t)q * out_stride, &n);
            out_counts[q] = n;
        }
    }
    if (fq.empty()) return WAX_HIP_OK;
    DeviceGuard g(e->device);
    ReadGuard rd(e);
    { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return frc; }
    return batch_filtered_locked(e, queries, nq, dims, clamp_topk(top_k), fq, F, n_allow_ids, min_scores, out_ids, out_scores, out_stride, out_counts, T);
}

int wax_hip_search_batch_predicate(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k,
                                   const uint64_t* allow_frame_ids, uint64_t n_allow_ids, const uint64_t* allow_begin,
                                   const uint64_t* allow_len, const float* min_scores, const wax_hip_row_predicate* preds,
                                   uint64_t* out_ids, float* out_scores, uint32_t out_stride, uint32_t* out_counts) {
    return search_batch_rows_entry(e, queries, nq, dims, top_k, allow_frame_ids, n_allow_ids, allow_begin, allow_len, min_scores, preds, nullptr, 0,
                                   nullptr, nullptr, out_ids, out_scores, out_stride, out_counts);
}

int wax_hip_search_batch_terms(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k,
                               const uint64_t* allow_frame_ids, uint64_t n_allow_ids, const uint64_t* allow_begin,
                               const uint64_t* allow_len, const float* min_scores, const wax_hip_row_predicate* preds,
                               const uint32_t* required_terms, uint64_t n_required_terms, const uint64_t* term_begin,
                               const uint32_t* term_len, uint64_t* out_ids, float* out_scores, uint32_t out_stride, uint32_t* out_counts) {
    return search_batch_rows_entry(e, queries, nq, dims, top_k, allow_frame_ids, n_allow_ids, allow_begin, allow_len, min_scores, preds, required_terms,
                                   n_required_terms, term_begin, term_len, out_ids, out_scores, out_stride, out_counts);
}

int wax_hip_search_batch_filtered(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k,
                                  const uint64_t* allow_frame_ids, uint64_t n_allow_ids, const uint64_t* allow_begin,
                                  const uint64_t* allow_len, const float* min_scores, uint64_t* out_ids, float* out_scores,
                                  uint32_t out_stride, uint32_t* out_counts) {
    return wax_hip_search_batch_predicate(e, queries, nq, dims, top_k, allow_frame_ids, n_allow_ids, allow_begin, allow_len, min_scores, nullptr,
                                          out_ids, out_scores, out_stride, out_counts);
}
