// api_terms.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: the per-row term column (set / get), its device copy, the required-term search, its read-out and the kernel's probe
// (DESIGN 4.11; FrameFilter.metadataFilter, SearchRequest.swift:130-145; matches(metadataFilter:meta:), UnifiedSearch.swift:1215-1239).
// The search itself is search_rows_locked (filter_host.inc) with the term mask in front of the attribute mask. The batched form
// (wax_hip_search_batch_terms) is filter_host.inc's batched body with a term set per entry; its term sets, the tables of
// term_mask_multi_kernel, its read-out and that kernel's probe are here.

// filter_host.inc
static inline bool predicate_is_empty(const wax_hip_row_predicate* p);
static inline wax_hip_row_predicate normalised_predicate(const wax_hip_row_predicate* p);

// The distinct required terms of one search, ascending.
struct TermReq {
    uint32_t n = 0;
    uint32_t t[TERMS_MAX_REQUIRED] = {};
};

// required[0 .. n) -> TermReq (duplicates collapse); false: more than TERMS_MAX_REQUIRED distinct terms
static bool make_term_req(const uint32_t* required, uint32_t n, TermReq* out) {
    std::vector<uint32_t> v(required, required + n);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    if (v.size() > (size_t)TERMS_MAX_REQUIRED) return false;
    out->n = (uint32_t)v.size();
    for (size_t i = 0; i < v.size(); ++i) out->t[i] = v[i];
    return true;
}

// The kernel's argument block: unused slots repeat the first term, so that a row passes exactly when all sixteen bits are set.
static void fill_term_mask_req(TermMaskArgs* a, const TermReq& req) {
    for (int i = 0; i < TERMS_MAX_REQUIRED; ++i) a->req[i] = req.t[(uint32_t)i < req.n ? i : 0];
}

// Does row r of the HOST column hold every required term? (the short allow-list's test: stage_host_rows)
static bool term_row_has_all(const wax_hip_engine* e, uint64_t r, const TermReq& req) {
    const TermColumn::Span set = e->cols.terms().span(r);          // behind the column: the empty set
    for (uint32_t i = 0; i < req.n; ++i)
        if (!std::binary_search(set.begin, set.end, req.t[i])) return false;
    return true;
}

// The term sets of one wax_hip_search_batch_terms call: the distinct sets in order of their first query (sets equal as sets are one),
// and each query's set (-1: no term filter).
struct BatchTerms {
    std::vector<TermReq> sets;
    std::vector<int32_t> of;
    const TermReq* req(uint32_t q) const { return of[q] >= 0 ? &sets[(size_t)of[q]] : nullptr; }
};

// The call's term arguments against themselves (no engine is looked at). *any = some query has a non-empty set.
static int make_batch_terms(uint32_t nq, const uint32_t* required_terms, uint64_t n_required_terms, const uint64_t* term_begin,
                            const uint32_t* term_len, BatchTerms* out, bool* any) {
    *any = false;
    if ((term_begin == nullptr) != (term_len == nullptr))
        return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "term_begin and term_len must both be given or both be null");
    if (!term_len) return WAX_HIP_OK;
    for (uint32_t q = 0; q < nq; ++q) {
        if (term_begin[q] > n_required_terms || term_len[q] > n_required_terms - term_begin[q])
            return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "term range of query " + std::to_string(q) + " leaves the term array");
        if (term_len[q] != 0 && !required_terms) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "required terms of query " + std::to_string(q) + " are null");
    }
    out->of.assign(nq, -1);
    std::map<std::vector<uint32_t>, int32_t> index;
    for (uint32_t q = 0; q < nq; ++q) {
        if (term_len[q] == 0) continue;
        TermReq r;
        if (!make_term_req(required_terms + term_begin[q], term_len[q], &r))
            return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "searchBatchTerms: query " + std::to_string(q) + " requires more than " +
                                                          std::to_string(TERMS_MAX_REQUIRED) + " distinct terms");
        auto it = index.emplace(std::vector<uint32_t>(r.t, r.t + r.n), (int32_t)out->sets.size());
        if (it.second) out->sets.push_back(r);
        out->of[q] = it.first->second;
        *any = true;
    }
    return WAX_HIP_OK;
}

// The tables of one term_mask_multi_kernel launch over sets[0 .. n_sets) (1 .. TERM_MULTI_MAX_SETS): the union of their terms ascending,
// padded with UINT32_MAX, then the membership words; the bit planes of the sets' sizes.
struct TermMultiPlan {
    uint32_t tables[2 * TERM_MULTI_MAX_UNION];
    uint32_t n_union;
    uint32_t nbits[5];
};
static void make_term_multi_plan(const TermReq* const* sets, uint32_t n_sets, TermMultiPlan* p) {
    std::vector<uint32_t> u;
    for (uint32_t s = 0; s < n_sets; ++s) u.insert(u.end(), sets[s]->t, sets[s]->t + sets[s]->n);
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    p->n_union = (uint32_t)u.size();
    for (uint32_t i = 0; i < TERM_MULTI_MAX_UNION; ++i) { p->tables[i] = i < u.size() ? u[i] : UINT32_MAX; p->tables[TERM_MULTI_MAX_UNION + i] = 0u; }
    for (uint32_t b = 0; b < 5; ++b) p->nbits[b] = 0u;
    for (uint32_t s = 0; s < n_sets; ++s) {
        for (uint32_t i = 0; i < sets[s]->n; ++i)
            p->tables[TERM_MULTI_MAX_UNION + (size_t)(std::lower_bound(u.begin(), u.end(), sets[s]->t[i]) - u.begin())] |= 1u << s;
        for (uint32_t b = 0; b < 5; ++b) p->nbits[b] |= ((sets[s]->n >> b) & 1u) << s;
    }
}

// ---- the column -------------------------------------------------------------------

// (TermPlan, one validated set_terms call, and TermRows, one store's share of it, are in row_columns.h with the column they are applied to)

static int validate_term_sets(const uint64_t* term_begin, const uint32_t* term_len, const uint32_t* terms, uint64_t n_terms, uint64_t n, TermPlan* p) {
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t len = term_len[i];
        if (term_begin[i] > n_terms || len > n_terms - term_begin[i])
            return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "setTerms: term range of entry " + std::to_string(i) + " leaves the term array");
        if (len != 0 && !terms) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "setTerms: term array is null");
        sum += len;
    }
    p->flat.resize((size_t)sum);
    p->e_off.assign((size_t)n + 1, 0);
    uint64_t w = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t len = term_len[i];
        uint32_t* b = p->flat.data() + w;
        if (len != 0) std::memcpy(b, terms + term_begin[i], (size_t)len * sizeof(uint32_t));
        std::sort(b, b + len);
        const uint64_t kept = (uint64_t)(std::unique(b, b + len) - b);
        if (kept > (uint64_t)TERMS_MAX_PER_ROW)
            return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "setTerms: entry " + std::to_string(i) + " holds more than " + std::to_string(TERMS_MAX_PER_ROW) + " distinct terms");
        w += kept;
        p->e_off[(size_t)i + 1] = w;
    }
    p->flat.resize((size_t)w);
    return WAX_HIP_OK;
}

int wax_hip_set_terms(wax_hip_engine* e, const uint64_t* frame_ids, const uint64_t* term_begin, const uint32_t* term_len, const uint32_t* terms,
                      uint64_t n_terms, uint64_t n, uint64_t* out_applied) {
    if (out_applied) *out_applied = 0;
    // the arguments against themselves first (no engine is looked at): nothing is applied when any entry is refused
    if (n != 0 && (!frame_ids || !term_begin || !term_len)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "setTerms: null input");
    TermPlan plan;
    { const int vrc = validate_term_sets(term_begin, term_len, terms, n_terms, n, &plan); if (vrc != WAX_HIP_OK) return vrc; }
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (n == 0) return WAX_HIP_OK;
    if (e->sh) return sh_set_terms(e, frame_ids, n, plan, out_applied);
    REFUSE_IF_HOLDING(e);
    WriteGuard w(e->lock);
    TermRows rows;
    uint64_t applied = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const int64_t r = e->idmap.find(frame_ids[i]);
        if (r < 0) continue;                                   // a frame without a vector has no row to describe
        ++applied;
        rows.emplace_back((uint64_t)r, i);
    }
    finish_term_rows(&rows);
    if (!rows.empty()) {
        if (e->cols.terms().total_after(plan, rows) >= 0x100000000ull) return fail(WAX_HIP_ERR_CAPACITY, "setTerms: the store would hold 2^32 terms or more");
        e->cols.commit_terms(plan, rows);
    }
    if (out_applied) *out_applied = applied;
    return WAX_HIP_OK;
}

int wax_hip_get_terms(wax_hip_engine* e, uint64_t frame_id, uint32_t* out_terms, uint32_t out_capacity, uint32_t* out_count, uint8_t* out_found) {
    if (out_count) *out_count = 0;
    if (out_found) *out_found = 0;
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (!out_count || (!out_terms && out_capacity)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "getTerms: null argument");
    if (e->sh) return sh_get_terms(e, frame_id, out_terms, out_capacity, out_count, out_found);
    ReadGuard rd(e);
    const int64_t r = e->idmap.find(frame_id);
    if (r < 0) return WAX_HIP_OK;
    if (out_found) *out_found = 1;
    const TermColumn::Span set = e->cols.terms().span((uint64_t)r);
    for (uint32_t i = 0; i < set.size() && i < out_capacity; ++i) out_terms[i] = set.begin[i];
    *out_count = set.size();
    return WAX_HIP_OK;
}

// The device CSR of the store as it is now (shared lock held; pending rows flushed; the host column is not empty): count + 1 offsets
// and the values. Concurrent term searches serialise here; what is uploaded is the offsets of rows [lowest changed or first
// appended, count] and the values from that row's offset on. Growth keeps what was current by a device copy.
static int ensure_terms(wax_hip_engine* e, hipStream_t st, const uint32_t** d_off, const uint32_t** d_val) {
    *d_off = nullptr; *d_val = nullptr;
    std::unique_lock<std::mutex> g(e->term_mu);
    const TermColumn& terms = e->cols.terms();
    UploadMark& mark = e->cols.term_mark();
    const uint64_t count = e->count, total = terms.total();
    uint64_t from = mark.from(count);
    bool current = mark.current(count);
    const uint64_t val_need = ((total + 3ull) & ~3ull) + 4ull;   // whole dwordx4 pieces (terms.hip), never an empty allocation
    if (e->term_off_cap < count + 1 || e->term_val_cap < val_need) {
        // the rows that were current are kept by a device copy, the rest is uploaded below
        const uint64_t keep = e->term_off_cap == 0 ? 0 : std::min(from, e->term_off_cap - 1);
        const uint64_t keep_val = std::min<uint64_t>(terms.offset(keep), e->term_val_cap);
        uint64_t off_cap = e->term_off_cap, val_cap = e->term_val_cap;
        if (off_cap < count + 1) off_cap = (e->capacity > count ? e->capacity : count) + 1;
        if (val_cap < val_need) { val_cap = std::max<uint64_t>(val_cap * 2, 1024); while (val_cap < val_need) val_cap *= 2; }
        uint32_t* no = nullptr;
        uint32_t* nv = nullptr;
        HIP_TRY(hipMalloc(&no, (size_t)off_cap * sizeof(uint32_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate the term offsets");
        hipError_t err = hipMalloc(&nv, (size_t)val_cap * sizeof(uint32_t));
        if (err == hipSuccess && keep > 0) err = hipMemcpyAsync(no, e->d_term_off, (size_t)keep * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
        if (err == hipSuccess && keep > 0 && keep_val > 0) err = hipMemcpyAsync(nv, e->d_term_val, (size_t)keep_val * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        if (err != hipSuccess) { (void)hipFree(no); (void)hipFree(nv); return fail(WAX_HIP_ERR_ALLOC, std::string("Failed to allocate the term values: ") + hipGetErrorString(err)); }
        (void)hipFree(e->d_term_off); (void)hipFree(e->d_term_val);
        e->d_term_off = no; e->d_term_val = nv; e->term_off_cap = off_cap; e->term_val_cap = val_cap;
        mark.note(keep);                                       // the new arrays hold nothing from there on
        from = mark.from(count);
        current = false;
    }
    if (!current) {
        // offsets of rows [from, count]: the host's, and the column's end for the rows behind it
        std::vector<uint32_t> offs((size_t)(count - from) + 1);
        for (uint64_t r = from; r <= count; ++r) offs[(size_t)(r - from)] = terms.offset(r);
        const uint32_t v0 = terms.offset(from);
        // pageable sources: the runtime stages them before returning
        HIP_TRY(hipMemcpyAsync(e->d_term_off + from, offs.data(), offs.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "term offset upload");
        if (v0 < total)
            HIP_TRY(hipMemcpyAsync(e->d_term_val + v0, terms.values() + v0, (size_t)(total - v0) * sizeof(uint32_t), hipMemcpyHostToDevice, st),
                    WAX_HIP_ERR_INTERNAL, "term value upload");
        HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "term upload failed on device");   // other workspaces' streams read the column next
        e->tm_rows_uploaded += count - from;
        e->tm_values_uploaded += total - v0;
    }
    mark.settle(count);
    *d_off = e->d_term_off; *d_val = e->d_term_val;
    return WAX_HIP_OK;
}

int wax_hip_term_stats(wax_hip_engine* e, wax_hip_term_stats_t* out) {
    if (!e || !out) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine/out is null");
    if (e->sh) return sh_term_stats(e, out);
    out->searches = e->tm_searches.load(); out->device_masks = e->tm_device_masks.load(); out->host_staged = e->tm_host_staged.load();
    out->host_decided = e->tm_host_decided.load(); out->term_rows_uploaded = e->tm_rows_uploaded.load();
    out->term_values_uploaded = e->tm_values_uploaded.load();
    return WAX_HIP_OK;
}

// ---- the search -------------------------------------------------------------------

int wax_hip_search_terms(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, int has_allow, const uint64_t* allow_frame_ids,
                         uint64_t n_allow, int has_min_score, float min_score, const wax_hip_row_predicate* pred, const uint32_t* required_terms,
                         uint32_t n_required, uint64_t* out_ids, float* out_scores, uint32_t out_capacity, uint32_t* out_count) {
    if (n_required == 0)   // no term to require: the predicate search as it is — one body, the same launches, the same counters
        return wax_hip_search_predicate(e, query, dims, top_k, has_allow, allow_frame_ids, n_allow, has_min_score, min_score, pred, out_ids, out_scores,
                                        out_capacity, out_count);
    // search_filtered_entry's refusals in its order, the new ones behind them
    if (out_count) *out_count = 0;
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (!query || !out_count || ((!out_ids || !out_scores) && out_capacity)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (has_allow && n_allow > 0 && !allow_frame_ids) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "allow-list is null");
    if (!e->sh && dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));
    if (!required_terms) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "required terms are null");
    TermReq req;
    if (!make_term_req(required_terms, n_required, &req))
        return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "searchTerms: more than " + std::to_string(TERMS_MAX_REQUIRED) + " distinct required terms");
    if (e->sh)
        return sh_search_terms(e, query, dims, top_k, has_allow, allow_frame_ids, n_allow, has_min_score, min_score, pred, req.t, req.n, out_ids,
                               out_scores, out_capacity, out_count);
    const wax_hip_row_predicate np = normalised_predicate(pred);
    uint32_t n = 0;
    {
        DeviceGuard g(e->device);
        ReadGuard rd(e);
        { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return frc; }
        e->tm_searches++;
        const int rc = search_rows_locked(e, query, dims, clamp_topk(top_k), has_allow, allow_frame_ids, n_allow, predicate_is_empty(&np) ? nullptr : &np,
                                          out_ids, out_scores, out_capacity, &n, &req);
        if (rc != WAX_HIP_OK) return rc;
    }
    if (has_min_score) apply_min_score(min_score, out_ids, out_scores, &n);
    *out_count = n;
    return WAX_HIP_OK;
}

// ---- the kernel's probe -----------------------------------------------------------

int wax_hip_term_mask_probe(const uint32_t* offsets, const uint32_t* values, uint64_t n_rows, const uint32_t* required, uint32_t n_required,
                            const uint32_t* bitmap_in, uint32_t grid, uint32_t* out_bitmap) {
    if (!offsets || !required || !out_bitmap) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (n_required == 0) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "term_mask_probe: at least one required term");
    TermReq req;
    if (!make_term_req(required, n_required, &req))
        return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "term_mask_probe: more than " + std::to_string(TERMS_MAX_REQUIRED) + " distinct required terms");
    if (grid == 0 || grid > TERM_MASK_MAX_GRID) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "term_mask_probe: 1 to 1024 workgroups");
    if (n_rows == 0 || n_rows > 0xffffffffull) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "term_mask_probe: 1 to 2^32 - 1 rows");
    for (uint64_t r = 0; r < n_rows; ++r)
        if (offsets[r] > offsets[r + 1]) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "term_mask_probe: offsets must not decrease");
    const uint64_t total = offsets[n_rows];
    if (total >= 0x80000000ull) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "term_mask_probe: fewer than 2^31 values");
    if (total != 0 && !values) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    const uint64_t n_words = (n_rows + 31) / 32;
    const uint64_t val_words = ((total + 3ull) & ~3ull) + 4ull, off_words = (n_rows + 1 + 3ull) & ~3ull;   // every section starts 16-byte aligned
    uint32_t* d = nullptr;
    HIP_TRY(hipMalloc(&d, (size_t)(val_words + off_words + n_words) * sizeof(uint32_t)), WAX_HIP_ERR_INTERNAL, "term_mask_probe allocation");
    uint32_t* d_val = d;
    uint32_t* d_off = d + val_words;
    uint32_t* d_bm = d_off + off_words;
    TermMaskArgs a{};
    a.off = d_off; a.val = d_val; a.bitmap = d_bm; a.n_rows = (uint32_t)n_rows; a.and_bitmap = bitmap_in ? 1 : 0;
    fill_term_mask_req(&a, req);
    hipError_t err = hipMemcpy(d_off, offsets, (size_t)(n_rows + 1) * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (err == hipSuccess && total != 0) err = hipMemcpy(d_val, values, (size_t)total * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (err == hipSuccess && bitmap_in) err = hipMemcpy(d_bm, bitmap_in, (size_t)n_words * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = launch_term_mask(a, grid, nullptr);
    if (err == hipSuccess) err = hipMemcpy(out_bitmap, d_bm, (size_t)n_words * sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIP_TRY(err, WAX_HIP_ERR_INTERNAL, "term_mask_probe");
    return WAX_HIP_OK;
}

int wax_hip_term_batch_stats(wax_hip_engine* e, wax_hip_term_batch_stats_t* out) {
    if (!e || !out) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine/out is null");
    if (e->sh) return sh_term_batch_stats(e, out);
    out->calls = e->tb_calls.load(); out->queries = e->tb_queries.load(); out->sets = e->tb_sets.load();
    out->mask_launches = e->tb_mask_launches.load(); out->looped = e->tb_looped.load(); out->host_decided = e->tb_host_decided.load();
    return WAX_HIP_OK;
}

int wax_hip_term_mask_multi_probe(const uint32_t* offsets, const uint32_t* values, uint64_t n_rows, const uint32_t* required,
                                  const uint64_t* set_begin, const uint32_t* set_len, uint32_t n_sets, uint32_t grid, uint32_t* out_bitmaps,
                                  uint32_t* out_counts) {
    if (!offsets || !required || !set_begin || !set_len || !out_bitmaps || !out_counts) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (n_sets == 0 || n_sets > TERM_MULTI_MAX_SETS) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "term_mask_multi_probe: 1 to 32 term sets");
    std::vector<TermReq> sets(n_sets);
    std::vector<const TermReq*> ptrs(n_sets);
    for (uint32_t s = 0; s < n_sets; ++s) {
        if (set_len[s] == 0) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "term_mask_multi_probe: set " + std::to_string(s) + " is empty");
        if (!make_term_req(required + set_begin[s], set_len[s], &sets[s]))
            return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "term_mask_multi_probe: set " + std::to_string(s) + " holds more than " +
                                                          std::to_string(TERMS_MAX_REQUIRED) + " distinct terms");
        ptrs[s] = &sets[s];
    }
    if (grid == 0 || grid > TERM_MASK_MAX_GRID) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "term_mask_multi_probe: 1 to 1024 workgroups");
    if (n_rows == 0 || n_rows > 0xffffffffull) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "term_mask_multi_probe: 1 to 2^32 - 1 rows");
    for (uint64_t r = 0; r < n_rows; ++r)
        if (offsets[r] > offsets[r + 1]) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "term_mask_multi_probe: offsets must not decrease");
    const uint64_t total = offsets[n_rows];
    if (total >= 0x80000000ull) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "term_mask_multi_probe: fewer than 2^31 values");
    if (total != 0 && !values) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    TermMultiPlan plan;
    make_term_multi_plan(ptrs.data(), n_sets, &plan);
    const uint64_t n_words = (n_rows + 31) / 32, stride = term_multi_stride_words((uint32_t)n_rows);
    const uint64_t val_words = ((total + 3ull) & ~3ull) + 4ull, off_words = (n_rows + 1 + 3ull) & ~3ull;   // every section starts 16-byte aligned
    const uint64_t table_words = 2ull * TERM_MULTI_MAX_UNION, count_words = TERM_MULTI_MAX_SETS;
    uint32_t* d = nullptr;
    HIP_TRY(hipMalloc(&d, (size_t)(val_words + off_words + table_words + count_words + stride * n_sets) * sizeof(uint32_t)), WAX_HIP_ERR_INTERNAL,
            "term_mask_multi_probe allocation");
    uint32_t* d_val = d;
    uint32_t* d_off = d_val + val_words;
    uint32_t* d_tab = d_off + off_words;
    uint32_t* d_cnt = d_tab + table_words;
    uint32_t* d_bm = d_cnt + count_words;
    TermMaskMultiArgs a{};
    a.off = d_off; a.val = d_val; a.uni = d_tab; a.memb = d_tab + TERM_MULTI_MAX_UNION; a.bitmaps = d_bm; a.counts = d_cnt;
    a.n_rows = (uint32_t)n_rows; a.n_union = plan.n_union; a.n_sets = n_sets; a.stride_words = (uint32_t)stride;
    for (int b = 0; b < 5; ++b) a.nbits[b] = plan.nbits[b];
    hipError_t err = hipMemcpy(d_off, offsets, (size_t)(n_rows + 1) * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (err == hipSuccess && total != 0) err = hipMemcpy(d_val, values, (size_t)total * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(d_tab, plan.tables, sizeof(plan.tables), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemset(d_cnt, 0, (size_t)count_words * sizeof(uint32_t));
    if (err == hipSuccess) err = launch_term_mask_multi(a, grid, nullptr);
    for (uint32_t s = 0; s < n_sets && err == hipSuccess; ++s)
        err = hipMemcpy(out_bitmaps + (size_t)s * n_words, d_bm + (size_t)s * stride, (size_t)n_words * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(out_counts, d_cnt, (size_t)n_sets * sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIP_TRY(err, WAX_HIP_ERR_INTERNAL, "term_mask_multi_probe");
    return WAX_HIP_OK;
}
