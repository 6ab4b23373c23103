// api_grouped.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: the parent column (set / get), the grouped search (PhotoRAGOrchestrator.swift:264-317, VideoRAGOrchestrator.swift:273-417:
// the `limit` best roots by their best member and the per_group best rows of each, selected on the device in one pass; grouped.hip,
// DESIGN 4.10), its read-out and a stateless probe of the selection.

// ---- the parent column ------------------------------------------------------------

int wax_hip_set_parents(wax_hip_engine* e, const uint64_t* frame_ids, const uint64_t* parent_ids, uint64_t n, uint64_t* out_applied) {
    if (out_applied) *out_applied = 0;
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (n == 0) return WAX_HIP_OK;
    if (!frame_ids || !parent_ids) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "setParents: null input");
    if (e->sh) return sh_set_parents(e, frame_ids, parent_ids, n, out_applied);
    REFUSE_IF_HOLDING(e);
    WriteGuard w(e->lock);
    uint64_t applied = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const int64_t r = e->idmap.find(frame_ids[i]);
        if (r < 0) continue;                                   // a frame without a vector has no row to describe
        ++applied;
        e->cols.set_parent((uint64_t)r, e->count, parent_ids[i]);
    }
    if (out_applied) *out_applied = applied;
    return WAX_HIP_OK;
}

int wax_hip_get_parents(wax_hip_engine* e, const uint64_t* frame_ids, uint64_t n, uint64_t* out_parents, uint8_t* out_found) {
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (n == 0) return WAX_HIP_OK;
    if (!frame_ids) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "getParents: null input");
    if (e->sh) return sh_get_parents(e, frame_ids, n, out_parents, out_found);
    ReadGuard rd(e);
    for (uint64_t i = 0; i < n; ++i) {
        const int64_t r = e->idmap.find(frame_ids[i]);
        if (out_parents) out_parents[i] = r >= 0 ? e->cols.parents().at((uint64_t)r) : WAX_HIP_NO_PARENT;
        if (out_found) out_found[i] = r >= 0 ? 1 : 0;
    }
    return WAX_HIP_OK;
}

// The group slots of the store as it is now (shared lock held; pending rows flushed): the device slot column, the root id of every slot
// and their number. A store without parents has neither column: slot = row, the roots are the frame ids (d_ids). Otherwise the host
// numbers the roots of rows [lowest changed or first appended, count) — a root it has seen keeps its slot, a new one takes the next —
// and uploads that range of the slot column and the new roots. Concurrent grouped searches serialise here. How roots are numbered is
// not part of the contract; that every row of one root shares a slot and no two roots do is.
static int ensure_groups(wax_hip_engine* e, hipStream_t st, const uint32_t** d_slots, const uint64_t** d_root, uint32_t* n_slots) {
    std::unique_lock<std::mutex> g(e->grp_mu);
    RowColumns& c = e->cols;
    const uint64_t count = e->count;
    if (c.parents().empty()) { *d_slots = nullptr; *d_root = e->d_ids; *n_slots = (uint32_t)count; return WAX_HIP_OK; }
    if (!c.groups_current(count)) {
        uint64_t from = c.number_groups(count, e->ids.data());
        if (e->grp_root_epoch != c.slots().epoch()) {              // numbering started over since the last upload: every root is sent again
            e->grp_root_epoch = c.slots().epoch();
            e->grp_root_dev = 0;
        }
        const uint64_t n_roots = c.slots().n_slots();
        if (e->grp_cap < count) {                                  // growth: the column is sent again whole
            const uint64_t cap = e->capacity > count ? e->capacity : count;
            (void)hipFree(e->d_grp_slot);
            e->d_grp_slot = nullptr; e->grp_cap = 0;
            HIP_TRY(hipMalloc(&e->d_grp_slot, (size_t)cap * sizeof(uint32_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate the group slot column");
            e->grp_cap = cap;
            from = 0;
        }
        if (e->grp_root_cap < n_roots) {
            uint64_t cap = 1024;
            while (cap < n_roots) cap *= 2;
            (void)hipFree(e->d_grp_root);
            e->d_grp_root = nullptr; e->grp_root_cap = 0; e->grp_root_dev = 0;
            HIP_TRY(hipMalloc(&e->d_grp_root, (size_t)cap * sizeof(uint64_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate the group root table");
            e->grp_root_cap = cap;
        }
        // pageable sources: the runtime stages them before returning
        if (from < count)
            HIP_TRY(hipMemcpyAsync(e->d_grp_slot + from, c.slots().slots() + from, (size_t)(count - from) * sizeof(uint32_t), hipMemcpyHostToDevice, st),
                    WAX_HIP_ERR_INTERNAL, "group slot upload");
        if (e->grp_root_dev < n_roots)
            HIP_TRY(hipMemcpyAsync(e->d_grp_root + e->grp_root_dev, c.slots().roots() + e->grp_root_dev,
                                   (size_t)(n_roots - e->grp_root_dev) * sizeof(uint64_t), hipMemcpyHostToDevice, st),
                    WAX_HIP_ERR_INTERNAL, "group root upload");
        HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "group slot upload failed on device");   // other workspaces' streams read the columns next
        e->grp_root_dev = n_roots;
        e->gs_parent_rows_uploaded += count - from;
    }
    c.group_mark().settle(count);
    *d_slots = e->d_grp_slot; *d_root = e->d_grp_root; *n_slots = (uint32_t)c.slots().n_slots();
    return WAX_HIP_OK;
}

// ---- the search ---------------------------------------------------------------------

// int64 words of one workspace buffer and where its parts begin (group_layout): everything a grouped search writes on the device.
struct GroupLayout {
    uint64_t tl, out, cur, best, dist_col, rank, dist, total;
};
static GroupLayout group_layout(uint64_t n_rows, uint32_t n_slots, int32_t limit, int32_t per_group) {
    GroupLayout l{};
    uint64_t at = 0;
    l.tl = at; at += timeline_scratch_words(timeline_grid(n_slots, limit), limit);
    l.out = at; at += group_out_words(limit, per_group);
    l.cur = at; at += 2ull * (uint64_t)limit;
    l.best = at; at += n_slots;
    l.dist_col = at; at += n_slots;
    l.rank = at; at += per_group > 0 ? ((uint64_t)n_slots + 1ull) / 2ull : 0ull;
    l.dist = at; at += (n_rows + 1ull) / 2ull;
    l.total = at;
    return l;
}

// One single-device engine's answer, raw: the out block of launch_group_select (kernels.h) for (limit, per_group), per_group 0 = no
// members. Takes the shared lock itself. `out` is resized; an empty engine, or a predicate nothing can pass, gives an all-padding block.
static int grouped_raw(wax_hip_engine* e, const float* query, uint32_t dims, int32_t limit, int32_t per_group, const wax_hip_row_predicate* pred,
                       std::vector<int64_t>& out) {
    const uint32_t L = (uint32_t)limit, P = (uint32_t)per_group;
    out.assign((size_t)group_out_words(limit, per_group), 0);
    for (uint32_t i = 0; i < L; ++i) out[i] = (int64_t)ID_PAD;
    for (uint32_t i = 0; i < L * P; ++i) { out[2u * L + 1u + i] = KEY_PAD; out[2u * L + 1u + L * P + i] = (int64_t)ID_PAD; }
    DeviceGuard g(e->device);
    ReadGuard rd(e);
    { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return frc; }
    if (e->count == 0) return WAX_HIP_OK;
    if (e->count > 0xffffffffull) return fail(WAX_HIP_ERR_CAPACITY, "count exceeds UInt32 row indices");
    const wax_hip_row_predicate np = normalised_predicate(pred);
    bool masked = !predicate_is_empty(&np);
    if (masked && !e->cols.has_attributes()) {                   // every row reads (0, 0): decided on the host
        if (!predicate_passes(np, 0, 0u)) return WAX_HIP_OK;
        masked = false;
    }
    FilterLease lease(e);
    if (lease.rc != WAX_HIP_OK) return lease.rc;
    FilterWork& f = lease.work();
    hipStream_t st = f.stream;
    const uint32_t count = (uint32_t)e->count;
    if (masked) {
        const int64_t* d_ts = nullptr;
        const uint32_t* d_fl = nullptr;
        { const int arc = ensure_attrs(e, st, &d_ts, &d_fl); if (arc != WAX_HIP_OK) return arc; }
        { const int grc = grow_dev(&f.d_bitmap, &f.bitmap_words, ((uint64_t)count + 31) / 32, sizeof(uint32_t), "Failed to allocate row bitmap"); if (grc != WAX_HIP_OK) return grc; }
        if (!f.d_pred_counts)
            HIP_TRY(hipMalloc(&f.d_pred_counts, kPredCounts * sizeof(uint32_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate predicate counters");
        AttrMaskArgs ma{};
        ma.ts = d_ts; ma.flags = d_fl; ma.bitmap = f.d_bitmap; ma.counts = f.d_pred_counts; ma.n_rows = count;
        ma.has_after = np.has_after; ma.has_before = np.has_before; ma.after = np.after; ma.before = np.before; ma.deny_flags = np.deny_flags;
        HIP_TRY(hipMemsetAsync(f.d_pred_counts, 0, kPredCounts * sizeof(uint32_t), st), WAX_HIP_ERR_INTERNAL, "predicate counters");
        HIP_TRY(launch_attr_mask(ma, st), WAX_HIP_ERR_INTERNAL, "attribute mask launch");
    }
    const uint32_t* d_slots = nullptr;
    const uint64_t* d_root = nullptr;
    uint32_t n_slots = 0;
    { const int grc = ensure_groups(e, st, &d_slots, &d_root, &n_slots); if (grc != WAX_HIP_OK) return grc; }
    const GroupLayout l = group_layout(count, n_slots, limit, per_group);
    { const int grc = grow_dev(&f.d_part, &f.part_cap, l.total, sizeof(int64_t), "Failed to allocate grouped-search scratch"); if (grc != WAX_HIP_OK) return grc; }
    int64_t* d = f.d_part;
    int64_t* d_best = d + l.best;
    float* d_dist = reinterpret_cast<float*>(d + l.dist);
    const bool fused = group_scan_dims(dims) && e->force_general.load() == 0;
    const bool want_dist = per_group > 1;
    HIP_TRY(launch_group_fill(d_best, n_slots, st), WAX_HIP_ERR_INTERNAL, "group fill launch");
    HIP_TRY(hipMemcpyAsync(f.d_query, query, (size_t)dims * sizeof(float), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "query upload");
    const float qn = query_norm(query, dims);
    if (fused) {
        GroupScanArgs a{};
        a.store = e->d_store; a.query = f.d_query; a.bitmap = masked ? f.d_bitmap : nullptr; a.slots = d_slots; a.best = d_best;
        a.dist_out = want_dist ? d_dist : nullptr; a.n_rows = count; a.n_slots = n_slots; a.dims = dims; a.q_norm = qn;
        HIP_TRY(launch_group_scan(a, e->metric, (int)e->grid_blocks.load(), st), WAX_HIP_ERR_INTERNAL, "grouped scan launch");
    } else {
        ScanArgs a{};
        a.store = e->d_store; a.query = f.d_query; a.dist_out = d_dist; a.n_rows = count; a.row_base = 0; a.dims = dims; a.k = 1; a.q_norm = qn;
        int grid = 0;
        HIP_TRY(launch_scan(a, e->metric, 0, 128, true, (int)e->grid_blocks.load(), st, &grid), WAX_HIP_ERR_INTERNAL, "distance scan launch");
        HIP_TRY(launch_group_offer(d_dist, d_slots, masked ? f.d_bitmap : nullptr, count, n_slots, d_best, 0u, st), WAX_HIP_ERR_INTERNAL, "group offer launch");
    }
    GroupSelectArgs s{};
    s.best = d_best; s.slot_root = d_root; s.dist = d_dist; s.slots = d_slots; s.bitmap = masked ? f.d_bitmap : nullptr; s.row_ids = e->d_ids;
    s.n_rows = count; s.n_slots = n_slots; s.limit = limit; s.per_group = per_group; s.grid = 0u;
    s.dist_col = d + l.dist_col; s.rank_of_slot = per_group > 0 ? reinterpret_cast<int32_t*>(d + l.rank) : nullptr; s.cur = d + l.cur;
    s.tl_scratch = d + l.tl; s.out = d + l.out;
    HIP_TRY(launch_group_select(s, st), WAX_HIP_ERR_INTERNAL, "group selection launch");
    static_assert((2ull * WAX_HIP_GROUP_MAX_LIMIT + 1ull + 2ull * WAX_HIP_GROUP_MAX_LIMIT * WAX_HIP_GROUP_MAX_MEMBERS) * sizeof(int64_t) <=
                      (size_t)WAX_HIP_MAX_RESULTS * sizeof(wax_hip_hit), "the pinned hit buffer holds a grouped answer");
    const size_t words = (size_t)group_out_words(limit, per_group);
    // without members the block's member parts were never written on the device: only the roots, the distances and the count come back
    const size_t copy_words = per_group > 0 ? words : 2u * (size_t)L + 1u;
    int64_t* h_out = reinterpret_cast<int64_t*>(f.h_hits);
    HIP_TRY(hipMemcpyAsync(h_out, d + l.out, copy_words * sizeof(int64_t), hipMemcpyDeviceToHost, st), WAX_HIP_ERR_INTERNAL, "grouped answer download");
    HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "grouped search failed on device");
    if (*reinterpret_cast<const uint32_t*>(h_out + 2u * (size_t)L) > L) return fail(WAX_HIP_ERR_INTERNAL, "grouped search: the device returned more groups than asked for");
    std::memcpy(out.data(), h_out, copy_words * sizeof(int64_t));
    e->gs_searches++;
    if (fused) e->gs_fused_scans++; else e->gs_column_scans++;
    if (per_group > 1) e->gs_member_rounds += (uint64_t)(per_group - 1);
    e->gs_group_slots = n_slots;
    e->st_searches++;
    e->st_rows += count;
    e->st_bytes += (uint64_t)count * dims * 4ull;
    return WAX_HIP_OK;
}

// VectorMetric.score(fromDistance:) (VectorMetric.swift:32-43), as hits_to_results applies it
static inline float group_score(uint8_t metric, float d) { return metric == WAX_HIP_METRIC_COSINE ? (1.0f - d) : (-d); }

// The argument checks every form shares; WAX_HIP_OK = go on.
static int grouped_refuse(wax_hip_engine* e, const float* query, int32_t limit, int32_t per_group, const uint64_t* out_root_ids,
                          const float* out_root_scores, const uint64_t* out_member_ids, const float* out_member_scores, const uint32_t* out_count) {
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (!query || !out_count || !out_root_ids || !out_root_scores) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if ((out_member_ids == nullptr) != (out_member_scores == nullptr)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "searchGrouped: member ids and scores come together");
    if (limit > WAX_HIP_GROUP_MAX_LIMIT) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "searchGrouped: limit exceeds WAX_HIP_GROUP_MAX_LIMIT (1024)");
    if (per_group > WAX_HIP_GROUP_MAX_MEMBERS) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "searchGrouped: per_group exceeds WAX_HIP_GROUP_MAX_MEMBERS (8)");
    return WAX_HIP_OK;
}

int wax_hip_search_grouped(wax_hip_engine* e, const float* query, uint32_t dims, int32_t limit, int32_t per_group, int has_min_score,
                           float min_score, const wax_hip_row_predicate* pred, uint64_t* out_root_ids, float* out_root_scores,
                           uint64_t* out_member_ids, float* out_member_scores, uint32_t* out_member_counts, uint32_t* out_count) {
    { const int rrc = grouped_refuse(e, query, limit, per_group, out_root_ids, out_root_scores, out_member_ids, out_member_scores, out_count); if (rrc != WAX_HIP_OK) return rrc; }
    if (dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));
    if (per_group < 1) per_group = 1;
    if (e->sh)
        return sh_search_grouped(e, query, dims, limit, per_group, has_min_score, min_score, pred, out_root_ids, out_root_scores, out_member_ids,
                                 out_member_scores, out_member_counts, out_count);
    *out_count = 0;
    if (limit <= 0) return WAX_HIP_OK;
    const bool members = out_member_ids != nullptr;
    const int32_t P = members ? per_group : 0;
    std::vector<int64_t> raw;
    { const int rc = grouped_raw(e, query, dims, limit, P, pred, raw); if (rc != WAX_HIP_OK) return rc; }
    const uint32_t L = (uint32_t)limit;
    const uint32_t n = *reinterpret_cast<const uint32_t*>(raw.data() + 2u * (size_t)L);
    const int64_t* keys = raw.data() + 2u * (size_t)L + 1u;
    const int64_t* mids = keys + (size_t)L * (uint32_t)P;
    uint32_t kept = 0;
    for (uint32_t gi = 0; gi < n; ++gi) {
        const float score = group_score(e->metric, unorder_bits((int32_t)raw[L + gi]));
        if (has_min_score && score < min_score) continue;       // `score < minScore` drops (UnifiedSearch.swift:1248); a NaN cut keeps everything
        out_root_ids[kept] = (uint64_t)raw[gi];
        out_root_scores[kept] = score;
        uint32_t m = 0;
        for (int32_t j = 0; j < P; ++j) {
            const int64_t k = keys[(size_t)gi * P + j];
            if (k == KEY_PAD) break;
            const float ms = group_score(e->metric, key_distance(k));
            if (has_min_score && ms < min_score) break;         // members are best-first: nothing behind it passes either
            out_member_ids[(size_t)kept * P + m] = (uint64_t)mids[(size_t)gi * P + j];
            out_member_scores[(size_t)kept * P + m] = ms;
            ++m;
        }
        for (int32_t j = (int32_t)m; j < P; ++j) { out_member_ids[(size_t)kept * P + j] = ID_PAD; out_member_scores[(size_t)kept * P + j] = 0.0f; }
        if (out_member_counts) out_member_counts[kept] = m;
        ++kept;
    }
    *out_count = kept;
    return WAX_HIP_OK;
}

int wax_hip_group_stats(wax_hip_engine* e, wax_hip_group_stats_t* out) {
    if (!e || !out) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (e->sh) return sh_group_stats(e, out);
    out->searches = e->gs_searches.load(); out->fused_scans = e->gs_fused_scans.load(); out->column_scans = e->gs_column_scans.load();
    out->member_rounds = e->gs_member_rounds.load(); out->group_slots = e->gs_group_slots.load();
    out->parent_rows_uploaded = e->gs_parent_rows_uploaded.load();
    return WAX_HIP_OK;
}

// ---- the probe ------------------------------------------------------------------------

int wax_hip_group_probe(const float* distances, const uint32_t* slots, const uint64_t* slot_root, const uint32_t* bitmap, uint64_t n_rows,
                        uint32_t n_slots, int32_t limit, int32_t per_group, uint32_t grid, uint64_t* out_root_ids, int64_t* out_root_keys,
                        int64_t* out_member_keys, uint32_t* out_count) {
    if (!out_root_ids || !out_root_keys || !out_count || (!distances && n_rows)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (limit > WAX_HIP_GROUP_MAX_LIMIT) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "group_probe: limit exceeds WAX_HIP_GROUP_MAX_LIMIT (1024)");
    if (per_group < 1 || per_group > WAX_HIP_GROUP_MAX_MEMBERS) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "group_probe: per_group must be 1 .. WAX_HIP_GROUP_MAX_MEMBERS");
    if (grid > 1024u) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "group_probe: at most 1024 workgroups");
    if (n_rows > 0xffffffffull) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "group_probe: at most 2^32 - 1 rows");
    if (!slots && (uint64_t)n_slots < n_rows) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "group_probe: without a slot column n_slots must cover the rows");
    if (slots)
        for (uint64_t r = 0; r < n_rows; ++r)
            if (slots[r] >= n_slots) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "group_probe: a slot is not below n_slots");
    *out_count = 0;
    if (limit <= 0) return WAX_HIP_OK;
    const uint32_t L = (uint32_t)limit, P = (uint32_t)per_group;
    for (uint32_t i = 0; i < L; ++i) { out_root_ids[i] = ID_PAD; out_root_keys[i] = KEY_PAD; }
    if (out_member_keys) for (uint32_t i = 0; i < L * P; ++i) out_member_keys[i] = KEY_PAD;
    if (n_rows == 0 || n_slots == 0) return WAX_HIP_OK;
    const GroupLayout l = group_layout(n_rows, n_slots, limit, per_group);
    const uint64_t slot_words = slots ? (n_rows + 1ull) / 2ull : 0ull, root_words = slot_root ? n_slots : 0ull;
    const uint64_t bm_n = (n_rows + 31ull) / 32ull, bm_words = bitmap ? (bm_n + 1ull) / 2ull : 0ull;
    int64_t* d = nullptr;
    HIP_TRY(hipMalloc(&d, (size_t)(l.total + slot_words + root_words + bm_words + 1ull) * sizeof(int64_t)), WAX_HIP_ERR_INTERNAL, "group_probe allocation");
    float* d_dist = reinterpret_cast<float*>(d + l.dist);
    uint32_t* d_slots = reinterpret_cast<uint32_t*>(d + l.total);
    uint64_t* d_root = reinterpret_cast<uint64_t*>(d + l.total + slot_words);
    uint32_t* d_bm = reinterpret_cast<uint32_t*>(d + l.total + slot_words + root_words);
    GroupSelectArgs s{};
    s.best = d + l.best; s.slot_root = slot_root ? d_root : nullptr; s.dist = d_dist; s.slots = slots ? d_slots : nullptr;
    s.bitmap = bitmap ? d_bm : nullptr; s.row_ids = nullptr; s.n_rows = (uint32_t)n_rows; s.n_slots = n_slots; s.limit = limit;
    s.per_group = per_group; s.grid = grid;
    s.dist_col = d + l.dist_col; s.rank_of_slot = reinterpret_cast<int32_t*>(d + l.rank); s.cur = d + l.cur; s.tl_scratch = d + l.tl; s.out = d + l.out;
    const size_t words = (size_t)group_out_words(limit, per_group);
    std::vector<int64_t> h((size_t)words);
    hipError_t err = hipMemcpy(d_dist, distances, (size_t)n_rows * sizeof(float), hipMemcpyHostToDevice);
    if (err == hipSuccess && slots) err = hipMemcpy(d_slots, slots, (size_t)n_rows * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (err == hipSuccess && slot_root) err = hipMemcpy(d_root, slot_root, (size_t)n_slots * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (err == hipSuccess && bitmap) err = hipMemcpy(d_bm, bitmap, (size_t)bm_n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = launch_group_fill(d + l.best, n_slots, nullptr);
    if (err == hipSuccess) err = launch_group_offer(d_dist, s.slots, s.bitmap, s.n_rows, n_slots, d + l.best, grid, nullptr);
    if (err == hipSuccess) err = launch_group_select(s, nullptr);
    if (err == hipSuccess) err = hipMemcpy(h.data(), d + l.out, words * sizeof(int64_t), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIP_TRY(err, WAX_HIP_ERR_INTERNAL, "group_probe");
    const uint32_t n = *reinterpret_cast<const uint32_t*>(h.data() + 2u * (size_t)L);
    if (n > L) return fail(WAX_HIP_ERR_INTERNAL, "group_probe: the device returned more groups than asked for");
    const int64_t* keys = h.data() + 2u * (size_t)L + 1u;
    for (uint32_t i = 0; i < n; ++i) { out_root_ids[i] = (uint64_t)h[i]; out_root_keys[i] = keys[(size_t)i * P]; }
    if (out_member_keys) std::memcpy(out_member_keys, keys, (size_t)L * P * sizeof(int64_t));
    *out_count = n;
    return WAX_HIP_OK;
}
