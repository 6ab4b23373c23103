// search_many.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: wax_hip_search_many and wax_hip_search_many_predicate (DESIGN 4.8) — one query each against many small stores of one device,
// answered under one snapshot: the eligible pairs by ONE pooled launch of the exact multi-query scan (multiscan.hip: every work item
// names its own store), one span merge that attaches each query's frame ids from its own engine's table, one download and one
// synchronisation; every other pair by the single-query search's body under the lock the call already holds. A pair may carry a row
// predicate and a score cut: the predicates of the pooled pairs become row bitmaps in one more launch ahead of the scan, which then
// offers only the rows whose bit is set. One body serves both entry points (search_many_impl).

// The pairs of one pooled engine that share a normalised predicate: they share passes over the store (up to 16 per pass) and, unless
// the predicate is empty, one row bitmap.
struct ManyClass {
    wax_hip_row_predicate pred{};
    bool masked = false;           // a non-empty predicate, evaluated on the device
    uint32_t word_off = 0;         // masked: the first word of its bitmap in the workspace's d_bitmap
    std::vector<uint32_t> pairs;   // indices into the call's arrays, in call order
};

// The pairs of one distinct engine, and how they are answered.
struct ManyEngine {
    wax_hip_engine* e;
    std::vector<uint32_t> pairs;   // indices into the call's arrays, in call order
    bool pooled = false;
    std::vector<ManyClass> classes;   // pooled, with rows: [0] is the empty predicate's class (no mask; it may hold no pair)
    const int64_t* d_ts = nullptr;    // the attribute columns, where a class is masked (ensure_attrs)
    const uint32_t* d_flags = nullptr;
    uint64_t passes(uint32_t group) const {   // the store is read once per group of up to `group` queries of one class
        uint64_t n = 0;
        for (const ManyClass& c : classes) n += (c.pairs.size() + group - 1) / group;
        return n;
    }
};

// The pooled pass over `pooled` (engines with rows, every one eligible), enqueued on the lease's stream: tables up in one copy, the
// row bitmaps of the masked classes (one launch, only when there is one), the scan, the merge, the hits' download into `hits`
// ([P][k], P = slot_q.size()). Nothing is synchronised here, and nothing comes back to the host before the hits: a mask that passes
// no row leaves KEY_PAD lists, which hits_to_results turns into count 0.
static int many_enqueue_pooled(std::vector<ManyEngine*>& pooled, FilterWork& f, const float* queries, uint32_t n, uint32_t dims,
                               int metric, int k, uint32_t group, int grid_cap, std::vector<uint32_t>& slot_q, std::vector<wax_hip_hit>& hits) {
    hipStream_t st = f.stream;
    // The masked classes' bitmaps, back to back in the workspace's d_bitmap (each starts on a word boundary), and the mask launch's
    // work table: one item per 256-row tile of a record.
    std::vector<AttrMaskRecord> records;
    std::vector<uint32_t> item_rec;
    uint64_t mask_words = 0;
    for (ManyEngine* m : pooled) {
        const uint32_t rows = (uint32_t)m->e->count;
        for (ManyClass& c : m->classes) {
            if (!c.masked || c.pairs.empty()) continue;
            c.word_off = (uint32_t)mask_words;
            AttrMaskRecord r{};
            r.ts = m->d_ts; r.flags = m->d_flags; r.n_rows = rows; r.word_off = c.word_off;
            r.has_after = c.pred.has_after; r.has_before = c.pred.has_before; r.after = c.pred.after; r.before = c.pred.before;
            r.deny_flags = c.pred.deny_flags; r.item0 = (uint32_t)item_rec.size();
            const uint32_t tiles = (uint32_t)(((uint64_t)rows + 255u) / 256u);
            item_rec.insert(item_rec.end(), tiles, (uint32_t)records.size());
            records.push_back(r);
            mask_words += ((uint64_t)rows + 31u) / 32u;
            if (mask_words >= 0x80000000ull || item_rec.size() >= 0x7fffffffull) return fail(WAX_HIP_ERR_CAPACITY, "too many masked rows in one call");
        }
    }
    const bool masked = !records.empty();
    if (masked) {   // (before the groups: they carry pointers into it)
        const int brc = grow_dev(&f.d_bitmap, &f.bitmap_words, mask_words, sizeof(uint32_t), "Failed to allocate search-many row bitmaps");
        if (brc != WAX_HIP_OK) return brc;
    }
    // Work split: the launch has about `grid_cap` work items (scan_multi_grid's cap: what one full-store pass would use). A group's
    // share of them is its share of the launch's chunks, at least one; within the share, scan_multi_grid's balanced split.
    uint64_t total_chunks = 0;
    for (const ManyEngine* m : pooled) total_chunks += scan_multi_chunks((uint32_t)m->e->count, dims) * m->passes(group);
    std::vector<PoolGroup> groups;
    std::vector<uint32_t> item_group, spans;
    std::vector<float> slot_norm;
    std::vector<MergeStore> stores;
    uint64_t part_lists = 0;
    for (const ManyEngine* m : pooled) {
        wax_hip_engine* e = m->e;
        const uint32_t rows = (uint32_t)e->count;
        const uint64_t share = (uint64_t)grid_cap * scan_multi_chunks(rows, dims) / (total_chunks ? total_chunks : 1);
        const uint32_t W = scan_multi_pooled_items(rows, dims, (uint32_t)(share < 1 ? 1 : share));
        for (const ManyClass& c : m->classes) {
            for (size_t g0 = 0; g0 < c.pairs.size(); g0 += group) {
                const uint32_t gn = (uint32_t)std::min<size_t>(group, c.pairs.size() - g0);
                PoolGroup G{};
                G.store = e->d_store; G.n_rows = rows; G.row_base = (uint32_t)e->row_base; G.q0 = (uint32_t)slot_q.size(); G.nq = gn;
                G.part_off = (uint32_t)part_lists; G.item0 = (uint32_t)item_group.size(); G.n_items = W;
                G.bitmap = c.masked ? f.d_bitmap + c.word_off : nullptr;
                for (uint32_t i = 0; i < gn; ++i) {
                    const uint32_t p = c.pairs[g0 + i];
                    slot_q.push_back(p);
                    slot_norm.push_back(query_norm(queries + (size_t)p * dims, dims));
                    spans.push_back((uint32_t)(part_lists + (uint64_t)i * W));
                    spans.push_back(W);
                    stores.push_back(MergeStore{e->d_ids, G.row_base, rows});
                }
                for (uint32_t w = 0; w < W; ++w) item_group.push_back((uint32_t)groups.size());
                groups.push_back(G);
                part_lists += (uint64_t)gn * W;
                if (part_lists >= 0x80000000ull / (uint64_t)k) return fail(WAX_HIP_ERR_CAPACITY, "too many partial lists in one call");
            }
        }
    }
    const uint32_t P = (uint32_t)slot_q.size();
    if (P == 0) return WAX_HIP_OK;               // every pair was answered on the host (predicates no row of an attribute-less store passes)
    // one blob: groups | item_group | slot_q | slot_norm | spans | stores | mask records | mask work table (16-byte aligned sections)
    auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t o_grp = 0, o_item = al(o_grp + groups.size() * sizeof(PoolGroup)), o_q = al(o_item + item_group.size() * 4);
    const size_t o_n = al(o_q + (size_t)P * 4), o_sp = al(o_n + (size_t)P * 4), o_st = al(o_sp + (size_t)P * 8);
    const size_t o_rec = al(o_st + (size_t)P * sizeof(MergeStore)), o_mi = al(o_rec + records.size() * sizeof(AttrMaskRecord));
    const size_t meta_bytes = al(o_mi + item_rec.size() * 4);
    std::vector<unsigned char> meta(meta_bytes, 0);
    std::memcpy(meta.data() + o_grp, groups.data(), groups.size() * sizeof(PoolGroup));
    std::memcpy(meta.data() + o_item, item_group.data(), item_group.size() * 4);
    std::memcpy(meta.data() + o_q, slot_q.data(), (size_t)P * 4);
    std::memcpy(meta.data() + o_n, slot_norm.data(), (size_t)P * 4);
    std::memcpy(meta.data() + o_sp, spans.data(), (size_t)P * 8);
    std::memcpy(meta.data() + o_st, stores.data(), (size_t)P * sizeof(MergeStore));
    if (masked) {
        std::memcpy(meta.data() + o_rec, records.data(), records.size() * sizeof(AttrMaskRecord));
        std::memcpy(meta.data() + o_mi, item_rec.data(), item_rec.size() * 4);
    }
    int grc = grow_dev(&f.d_meta, &f.meta_cap, meta_bytes, 1, "Failed to allocate search-many tables");
    if (grc == WAX_HIP_OK) grc = grow_dev(&f.d_bq, &f.bq_cap, (uint64_t)n * dims, sizeof(float), "Failed to allocate search-many queries");
    if (grc == WAX_HIP_OK) grc = grow_dev(&f.d_part, &f.part_cap, part_lists * (uint64_t)k, sizeof(int64_t), "Failed to allocate search-many partials");
    if (grc == WAX_HIP_OK) grc = grow_dev(&f.d_bhits, &f.bhits_cap, (uint64_t)P * k, sizeof(wax_hip_hit), "Failed to allocate search-many hits");
    if (grc != WAX_HIP_OK) return grc;
    HIP_TRY(hipMemcpyAsync(f.d_bq, queries, (size_t)n * dims * sizeof(float), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "query upload");
    HIP_TRY(hipMemcpyAsync(f.d_meta, meta.data(), meta_bytes, hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "search-many table upload");
    ScanMultiArgs a{};
    a.queries = f.d_bq;
    a.qlist = reinterpret_cast<const uint32_t*>(f.d_meta + o_q);
    a.q_norm = reinterpret_cast<const float*>(f.d_meta + o_n);
    a.partials = f.d_part;
    a.dims = dims; a.k = k;
    a.item_group = reinterpret_cast<const uint32_t*>(f.d_meta + o_item);
    if (masked) {
        HIP_TRY(launch_attr_mask_pooled(reinterpret_cast<const AttrMaskRecord*>(f.d_meta + o_rec), reinterpret_cast<const uint32_t*>(f.d_meta + o_mi),
                                        (uint32_t)item_rec.size(), f.d_bitmap, st), WAX_HIP_ERR_INTERNAL, "pooled attribute mask launch");
        HIP_TRY(launch_scan_multi_pooled_masked(a, reinterpret_cast<const PoolGroup*>(f.d_meta + o_grp), metric, (uint32_t)item_group.size(), st),
                WAX_HIP_ERR_INTERNAL, "pooled masked scan launch");
    } else {
        HIP_TRY(launch_scan_multi_pooled(a, reinterpret_cast<const PoolGroup*>(f.d_meta + o_grp), metric, (uint32_t)item_group.size(), st),
                WAX_HIP_ERR_INTERNAL, "pooled scan launch");
    }
    HIP_TRY(launch_merge_keys_stores(f.d_part, reinterpret_cast<const uint32_t*>(f.d_meta + o_sp), reinterpret_cast<const MergeStore*>(f.d_meta + o_st), k,
                                     f.d_bhits, (uint32_t)k, P, st), WAX_HIP_ERR_INTERNAL, "pooled merge launch");
    hits.resize((size_t)P * k);
    HIP_TRY(hipMemcpyAsync(hits.data(), f.d_bhits, hits.size() * sizeof(wax_hip_hit), hipMemcpyDeviceToHost, st), WAX_HIP_ERR_INTERNAL, "hits download");
    return WAX_HIP_OK;
}

// wax_hip_search_many (preds == min_scores == nullptr) and wax_hip_search_many_predicate.
static int search_many_impl(wax_hip_engine* const* engines, const float* queries, uint32_t n, uint32_t dims, int32_t top_k,
                            const wax_hip_row_predicate* preds, const float* min_scores, uint64_t* out_ids, float* out_scores,
                            uint32_t out_stride, uint32_t* out_counts) {
    if (n == 0) return WAX_HIP_OK;
    if (!engines) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine list is null");
    // every refusal comes before any lock, launch or write to the outputs, and names the pair
    for (uint32_t i = 0; i < n; ++i) {
        const wax_hip_engine* e = engines[i];
        const std::string who = "pair " + std::to_string(i) + ": ";
        if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, who + "engine is null");
        if (e->sh) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, who + "wax_hip_search_many takes single-device engines, not a sharded handle");
        if (e->device != engines[0]->device)
            return fail(WAX_HIP_ERR_INVALID_ARGUMENT, who + "engine is on device " + std::to_string(e->device) + ", pair 0's on device " +
                                                          std::to_string(engines[0]->device) + " (one device per call)");
        if (e->metric != engines[0]->metric) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, who + "engine's metric differs from pair 0's (one metric per call)");
        if (e->dims != dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, who + dim_mismatch_msg(e->dims, dims));
    }
    if (!queries || !out_counts) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null input");
    if ((!out_ids || !out_scores) && out_stride) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "output arrays are null");
    for (uint32_t i = 0; i < n; ++i) out_counts[i] = 0;
    if (out_stride == 0) return WAX_HIP_OK;

    // distinct engines in ascending address order: the order their locks are taken in (two calls listing the same engines in opposite
    // orders, and writers that each hold one exclusive lock and wait for nothing else, cannot form a cycle)
    std::vector<ManyEngine> many;
    {
        std::vector<wax_hip_engine*> distinct(engines, engines + n);
        std::sort(distinct.begin(), distinct.end(), std::less<wax_hip_engine*>());
        distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
        many.resize(distinct.size());
        for (size_t j = 0; j < distinct.size(); ++j) many[j].e = distinct[j];
        for (uint32_t i = 0; i < n; ++i) {
            const size_t j = (size_t)(std::lower_bound(distinct.begin(), distinct.end(), engines[i], std::less<wax_hip_engine*>()) - distinct.begin());
            many[j].pairs.push_back(i);
        }
    }
    const int metric = engines[0]->metric;
    DeviceGuard g(engines[0]->device);
    std::vector<std::unique_ptr<ReadGuard>> locks;   // one snapshot: every distinct engine's shared lock, held to the end of the call
    locks.reserve(many.size());
    for (ManyEngine& m : many) {
        locks.emplace_back(new ReadGuard(m.e));
        const int frc = flush_pending(m.e);          // a row staged just before the call is in the answer
        if (frc != WAX_HIP_OK) return frc;
    }

    // ---- route ----
    const int kpad = clamp_topk(top_k);
    const uint32_t group = kpad <= FUSED_MAX_K ? scan_multi_group(dims, kpad) : 0u;
    std::vector<ManyEngine*> pooled;
    bool any_masked = false;
    for (ManyEngine& m : many) {
        wax_hip_engine* e = m.e;
        m.pooled = group != 0 && e->search_many.load() != 0 && e->force_general.load() == 0 &&
                   e->count <= (uint64_t)e->search_many_max_rows.load() && e->row_base + e->count <= 0x100000000ull;
        if (!m.pooled) continue;
        e->st_many_pooled += m.pairs.size();
        e->st_searches += m.pairs.size();
        // The pairs by normalised predicate. A store that never had attributes has no columns to read (ensure_attrs: every row is
        // (0, 0)): its predicates are decided here, once for all rows — the pair is an unmasked pair, or its count stays 0.
        const bool has_attrs = e->cols.has_attributes();
        typedef std::tuple<int32_t, int64_t, int32_t, int64_t, uint32_t> PredKey;
        std::map<PredKey, size_t> index;
        m.classes.emplace_back();                    // [0]: no predicate, no mask
        uint64_t n_masked = 0;
        for (uint32_t p : m.pairs) {
            const wax_hip_row_predicate np = normalised_predicate(preds ? &preds[p] : nullptr);
            if (predicate_is_empty(&np)) { m.classes[0].pairs.push_back(p); continue; }
            e->st_predicate_searches++;
            if (!has_attrs) {
                if (predicate_passes(np, 0, 0u)) m.classes[0].pairs.push_back(p);
                continue;
            }
            if (e->count == 0) continue;
            const auto it = index.emplace(PredKey(np.has_after, np.after, np.has_before, np.before, np.deny_flags), m.classes.size());
            if (it.second) { m.classes.emplace_back(); m.classes.back().pred = np; m.classes.back().masked = true; }
            m.classes[it.first->second].pairs.push_back(p);
            ++n_masked;
        }
        if (e->count == 0) continue;                 // an empty store: count 0, nothing to launch
        // every group reads the whole store once — a masked group too: its row loads are unconditional (multiscan_body.inc)
        const uint64_t passes = m.passes(group);
        if (passes == 0) continue;                   // every pair was decided on the host
        e->st_rows += e->count * passes;
        e->st_bytes += e->count * passes * (uint64_t)dims * 4ull;
        e->st_many_masked += n_masked;
        any_masked = any_masked || n_masked != 0;
        pooled.push_back(&m);
    }

    // ---- the pooled pass, on a workspace leased from the first pooled engine's pool ----
    // (A looped engine is never the lease's host engine — an engine is pooled or looped as a whole — so the workspace its own
    // predicate search leases below comes from another engine's pool and cannot wait on this one.)
    std::unique_ptr<FilterLease> lease;
    std::vector<uint32_t> slot_q;
    std::vector<wax_hip_hit> hits;
    if (!pooled.empty()) {
        wax_hip_engine* host = pooled[0]->e;
        lease.reset(new FilterLease(host));
        if (lease->rc != WAX_HIP_OK) return lease->rc;
        if (any_masked) {
            // the attribute columns of every engine with a masked class, brought up to date on the lease's stream under the lock held
            // (a synchronisation only where columns changed since the engine's last predicate search)
            for (ManyEngine* m : pooled) {
                bool need = false;
                for (const ManyClass& c : m->classes) need = need || (c.masked && !c.pairs.empty());
                if (!need) continue;
                const int arc = ensure_attrs(m->e, lease->work().stream, &m->d_ts, &m->d_flags);
                if (arc != WAX_HIP_OK) return arc;
            }
        }
        const int64_t gb = host->grid_blocks.load();
        const int grid_cap = gb <= 0 ? 512 : (gb > MAX_GRID_BLOCKS ? MAX_GRID_BLOCKS : (int)gb);
        const int prc = many_enqueue_pooled(pooled, lease->work(), queries, n, dims, metric, kpad, group, grid_cap, slot_q, hits);
        if (prc != WAX_HIP_OK) return prc;           // (the lease's destructor drains the stream)
    }

    // ---- every other pair: the single-query search's body, under the lock already held (it overlaps the pooled pass) ----
    for (ManyEngine& m : many) {
        if (m.pooled) continue;
        for (uint32_t p : m.pairs) {
            const wax_hip_row_predicate np = normalised_predicate(preds ? &preds[p] : nullptr);
            int rc;
            if (!predicate_is_empty(&np)) {
                rc = search_rows_locked(m.e, queries + (size_t)p * dims, dims, kpad, /*has_allow=*/0, nullptr, 0, &np, out_ids + (size_t)p * out_stride,
                                        out_scores + (size_t)p * out_stride, out_stride, &out_counts[p]);
            } else {
                uint64_t t = 0;
                rc = submit_impl(m.e, queries + (size_t)p * dims, dims, top_k, &t, /*try_only=*/false, /*caller_locked=*/true);
                if (rc == WAX_HIP_OK)
                    rc = collect_impl(m.e, t, out_ids + (size_t)p * out_stride, out_scores + (size_t)p * out_stride, out_stride, &out_counts[p], nullptr, 0,
                                      /*caller_locked=*/true);
            }
            if (rc != WAX_HIP_OK) return rc;
            m.e->st_many_looped++;
        }
    }

    // ---- one synchronisation, then the hits on the host ----
    if (!slot_q.empty()) {
        HIP_TRY(hipStreamSynchronize(lease->work().stream), WAX_HIP_ERR_INTERNAL, "search-many failed on device");
        for (size_t s = 0; s < slot_q.size(); ++s) {
            const uint32_t p = slot_q[s];
            hits_to_results((uint8_t)metric, hits.data() + s * (size_t)kpad, (uint32_t)kpad, out_ids + (size_t)p * out_stride,
                            out_scores + (size_t)p * out_stride, out_stride, &out_counts[p]);
        }
    }
    // the score cut, per pair, on whatever route answered it
    if (min_scores)
        for (uint32_t i = 0; i < n; ++i) apply_min_score(min_scores[i], out_ids + (size_t)i * out_stride, out_scores + (size_t)i * out_stride, &out_counts[i]);
    return WAX_HIP_OK;
}

int wax_hip_search_many(wax_hip_engine* const* engines, const float* queries, uint32_t n, uint32_t dims, int32_t top_k,
                        uint64_t* out_ids, float* out_scores, uint32_t out_stride, uint32_t* out_counts) {
    return search_many_impl(engines, queries, n, dims, top_k, nullptr, nullptr, out_ids, out_scores, out_stride, out_counts);
}

int wax_hip_search_many_predicate(wax_hip_engine* const* engines, const float* queries, uint32_t n, uint32_t dims, int32_t top_k,
                                  const wax_hip_row_predicate* preds, const float* min_scores, uint64_t* out_ids, float* out_scores,
                                  uint32_t out_stride, uint32_t* out_counts) {
    return search_many_impl(engines, queries, n, dims, top_k, preds, min_scores, out_ids, out_scores, out_stride, out_counts);
}
