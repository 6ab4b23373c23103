// batch_host.inc — part of engine.hip's translation unit (included there; not compiled alone).
// batched queries, host side: the incremental bf16 mirror and id table, pooled batch workspaces, the one-pass planner, the launch chain (`batch_enqueue`) and the exactness ladder behind it (DESIGN 4.4)

// ---------------------------------------------------------------------------
// Batched path: Q x D^T on the matrix cores (batch.hip). Everything here is called with the shared lock held.

// Rows the next ensure_mirror would convert (a planning figure: read without the mirror's mutex).
static double mirror_rows_to_convert(wax_hip_engine* e) {
    const BatchMirror& b = e->batch;
    if (e->derived.bf16.current()) return 0.0;
    if (b.d_cb == nullptr || b.mirror_cap < e->capacity) return (double)e->count;
    return (double)e->derived.bf16.pending(e->count);
}

// remove(frameId:) moved store rows (idx, count) down by one (MetalVectorEngine.swift:431-438): where the mirror holds row idx its tail
// follows (half the bytes of the store's own move). Device work only, called BEFORE count is decremented; anything but WAX_HIP_OK = the
// mirror could not follow. (A fill that holds a row has a buffer: the fill only leaves its restart in ensure_mirror, behind the
// allocation for a capacity of at least count rows, and d_cb is only ever replaced by a larger buffer.)
static int mirror_follow_remove(wax_hip_engine* e, uint64_t idx) {
    BatchMirror& b = e->batch;
    if (!e->derived.bf16.holds(idx)) return WAX_HIP_OK;
    if (b.ev_pending) { (void)hipEventSynchronize(b.ev_ready); b.ev_pending = false; }
    const uint64_t after = e->derived.bf16.rows() - 1 - idx;
    if (after > 0) {
        if (!e->d_bounce)
            HIP_TRY(hipMalloc(&e->d_bounce, kBounceBytes), WAX_HIP_ERR_ALLOC, "Failed to allocate bounce buffer");
        const uint64_t rb = (uint64_t)e->dims * sizeof(unsigned short);
        HIP_TRY(device_shift_down(b.d_cb, idx * rb, (idx + 1) * rb, after * rb, e->d_bounce, kBounceBytes, nullptr), WAX_HIP_ERR_INTERNAL, "mirror row shift");
        HIP_TRY(device_shift_down(b.d_vn2, idx * 4, (idx + 1) * 4, after * 4, e->d_bounce, kBounceBytes, nullptr), WAX_HIP_ERR_INTERNAL, "mirror norm shift");
        HIP_TRY(hipStreamSynchronize(nullptr), WAX_HIP_ERR_INTERNAL, "mirror shift sync");
    }
    return WAX_HIP_OK;
}

// removeBatch: the rows `rem` (ascending, distinct) leave the store in one compaction pass (compact.hip; DESIGN 4.7). `mirror_rows`
// > 0 = the mirror and its norms follow, rows below that fill. Enqueues on the null stream and waits for it; *bytes_written = device
// bytes the pass wrote, bounce writes included. Nothing on the host side is touched here. Called BEFORE count drops.
static int compact_removed_rows(wax_hip_engine* e, const std::vector<uint32_t>& rem, const uint32_t* d_rem, uint64_t mirror_rows,
                                uint64_t* bytes_written) {
    const uint32_t m = (uint32_t)rem.size();
    const uint64_t count = e->count;
    const uint32_t D = e->dims;
    BatchMirror& b = e->batch;
    struct Arr { char* base; uint64_t rb; uint64_t limit; uint64_t rank_limit; uint64_t sect; };
    Arr arrs[kCompactMaxArrays];
    int na = 0;
    arrs[na++] = Arr{reinterpret_cast<char*>(e->d_store), (uint64_t)D * sizeof(float), count, m, 0};
    arrs[na++] = Arr{reinterpret_cast<char*>(e->d_ids), sizeof(uint64_t), count, m, 0};
    if (mirror_rows > 0) {
        const uint64_t pl = (uint64_t)(std::lower_bound(rem.begin(), rem.end(), (uint32_t)std::min<uint64_t>(mirror_rows, 0xffffffffull)) - rem.begin());
        arrs[na++] = Arr{reinterpret_cast<char*>(b.d_cb), (uint64_t)D * sizeof(unsigned short), mirror_rows, pl, 0};
        arrs[na++] = Arr{reinterpret_cast<char*>(b.d_vn2), sizeof(float), mirror_rows, pl, 0};
    }
    // window = as many source rows as the bounce buffer holds of all arrays at once (each array has its own 256-byte-aligned section)
    uint64_t per_row = 0;
    for (int i = 0; i < na; ++i) per_row += arrs[i].rb;
    uint64_t window = (kBounceBytes - 256ull * kCompactMaxArrays) / per_row;
    if (window < 1) return fail(WAX_HIP_ERR_CAPACITY, "removeBatch: one row of every per-row array does not fit the bounce buffer");
    const uint64_t want = (uint64_t)e->compact_window_rows.load();
    if (want > 0 && want < window) window = want;
    {
        uint64_t off = 0;
        for (int i = 0; i < na; ++i) { arrs[i].sect = off; off += (window * arrs[i].rb + 255ull) & ~255ull; }
    }
    const bool nt = (count - rem[0]) * arrs[0].rb > (64ull << 20);    // the tail is streamed once: keep it out of the caches when it is far larger than L2
    char* bounce = static_cast<char*>(e->d_bounce);
    uint64_t written = 0;
    uint64_t w0 = rem[0];
    uint32_t p = 0;
    for (;;) {
        while (p < m && rem[p] == w0) { ++p; ++w0; }                  // a window starts at a surviving row
        if (w0 >= count) break;
        const uint64_t shift = p;                                     // rank(w0) >= 1
        const bool direct = shift >= window;                          // destination [w0 - shift, ...) ends at or below w0 for len <= shift
        const uint64_t len = direct ? shift : window;
        const uint64_t w1 = std::min<uint64_t>(count, w0 + len);
        const uint32_t p1 = (uint32_t)(std::lower_bound(rem.begin() + p, rem.end(), (uint32_t)std::min<uint64_t>(w1, 0xffffffffull)) - rem.begin());
        const uint64_t dst0 = w0 - shift;
        RowCompactArgs a{};
        a.rem = d_rem; a.p0 = p; a.p1 = p1; a.w0 = (uint32_t)w0; a.w1 = (uint32_t)w1; a.dst0 = (uint32_t)dst0;
        uint64_t surv[kCompactMaxArrays];
        int idx[kCompactMaxArrays];
        for (int i = 0; i < na; ++i) {
            const Arr& r = arrs[i];
            if (r.limit <= w0) continue;                              // (the mirror ends below this window)
            const uint64_t end = std::min(w1, r.limit);
            const uint64_t rank_end = r.limit >= w1 ? p1 : r.rank_limit;
            const int j = a.n_arrays++;
            idx[j] = i;
            surv[j] = (end - rank_end) - dst0;
            a.arr[j].src = r.base;
            a.arr[j].out = direct ? r.base + dst0 * r.rb : bounce + r.sect;
            a.arr[j].row_bytes = (uint32_t)r.rb;
            a.arr[j].limit = (uint32_t)std::min<uint64_t>(r.limit, 0xffffffffull);
        }
        HIP_TRY(launch_compact_rows(a, nt, nullptr), WAX_HIP_ERR_INTERNAL, "row compaction launch");
        for (int j = 0; j < a.n_arrays; ++j) {
            const Arr& r = arrs[idx[j]];
            const uint64_t bytes = surv[j] * r.rb;
            written += bytes;
            if (direct || bytes == 0) continue;
            HIP_TRY(hipMemcpyAsync(r.base + dst0 * r.rb, bounce + r.sect, bytes, hipMemcpyDeviceToDevice, nullptr), WAX_HIP_ERR_INTERNAL, "row compaction copy");
            written += bytes;
        }
        w0 = w1;
        p = p1;
    }
    HIP_TRY(hipStreamSynchronize(nullptr), WAX_HIP_ERR_INTERNAL, "row compaction sync");
    *bytes_written = written;
    return WAX_HIP_OK;
}

// The bf16 mirror of the store (+ ||v||^2, max ||v||, max rounding error): allocated at the first batched search, then kept in step
// with the store incrementally — see BatchMirror. Concurrent batches serialise on the conversion's ENQUEUE only: nothing here waits
// for the device (the converting stream records an event that every other workspace's stream waits for).
int ensure_mirror(wax_hip_engine* e, hipStream_t st) {
    BatchMirror& b = e->batch;
    DirtyRowFill& fill = e->derived.bf16;
    if (fill.current() && b.mirror_cap >= e->capacity) {
        // converted, but perhaps still in flight on another workspace's stream
        std::unique_lock<std::mutex> g(b.mu);
        if (b.ev_pending) {
            if (hipEventQuery(b.ev_ready) == hipSuccess) b.ev_pending = false;
            else HIP_TRY(hipStreamWaitEvent(st, b.ev_ready, 0), WAX_HIP_ERR_INTERNAL, "mirror ready wait");
        }
        return WAX_HIP_OK;
    }
    std::unique_lock<std::mutex> g(b.mu);
    const uint32_t D = e->dims;
    if (!b.d_maxnorm) {
        HIP_TRY(hipMalloc(&b.d_maxnorm, 2 * sizeof(unsigned int)), WAX_HIP_ERR_ALLOC, "Failed to allocate batch scalars");
        HIP_TRY(hipMalloc(&b.d_dirty, kMirrorMaxDirty * sizeof(uint32_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate batch scalars");
        HIP_TRY(hipEventCreateWithFlags(&b.ev_ready, hipEventDisableTiming), WAX_HIP_ERR_INTERNAL, "event create");
    }
    if (b.ev_pending) HIP_TRY(hipStreamWaitEvent(st, b.ev_ready, 0), WAX_HIP_ERR_INTERNAL, "mirror ready wait");   // order behind the previous conversion
    if (b.mirror_cap < e->capacity) {
        // The store was reallocated (capacity doubles, MetalVectorEngine.swift:857-871). No batch can be reading the old mirror: a
        // smaller mirror is only possible after a mutation, which took the exclusive lock after every reader had finished. The
        // converted rows move over (a device copy of half the store's bytes, not a re-conversion from f32).
        unsigned short* ncb = nullptr; float* nvn = nullptr;
        // + slack rows: the filtering GEMM requests whole tiles without clamps — its last tile may run up to (tile rows - 1) rows
        // past the store, plus one row for the pad slots and the slack behind the tile image (never used: masked by the selection)
        HIP_TRY(hipMalloc(&ncb, ((size_t)e->capacity + BATCH_MIRROR_SLACK_ROWS) * D * sizeof(unsigned short)), WAX_HIP_ERR_ALLOC, "Failed to allocate bf16 mirror");
        if (hipMalloc(&nvn, (size_t)e->capacity * sizeof(float)) != hipSuccess) { (void)hipFree(ncb); return fail(WAX_HIP_ERR_ALLOC, "Failed to allocate row norms"); }
        hipError_t err = hipMemsetAsync(ncb + (size_t)e->capacity * D, 0, (size_t)BATCH_MIRROR_SLACK_ROWS * D * sizeof(unsigned short), st);
        const uint64_t kept = fill.restarting() ? 0 : fill.rows();
        if (err == hipSuccess && kept > 0 && b.d_cb) {
            err = hipMemcpyAsync(ncb, b.d_cb, (size_t)kept * D * sizeof(unsigned short), hipMemcpyDeviceToDevice, st);
            if (err == hipSuccess) err = hipMemcpyAsync(nvn, b.d_vn2, (size_t)kept * sizeof(float), hipMemcpyDeviceToDevice, st);
            if (err == hipSuccess) err = hipStreamSynchronize(st);                     // the old buffers are freed next
        } else {
            fill.restart();
        }
        if (err != hipSuccess) { (void)hipFree(ncb); (void)hipFree(nvn); return fail(WAX_HIP_ERR_INTERNAL, std::string("mirror move: ") + hipGetErrorString(err)); }
        (void)hipFree(b.d_cb); (void)hipFree(b.d_vn2);
        b.d_cb = ncb; b.d_vn2 = nvn; b.mirror_cap = e->capacity;
    }
    const uint64_t count = e->count;
    const RowFill::Build build = fill.begin(count);
    if (build.scratch) HIP_TRY(hipMemsetAsync(b.d_maxnorm, 0, 2 * sizeof(unsigned int), st), WAX_HIP_ERR_INTERNAL, "batch memset");
    const int normalize = e->metric == WAX_HIP_METRIC_COSINE ? 1 : 0;
    uint64_t converted = 0;
    if (build.from < count) {                                 // appended since: rows [from, count)
        const uint64_t n_new = count - build.from;
        HIP_TRY(launch_mirror(e->d_store + build.from * D, (uint32_t)n_new, (uint32_t)n_new, D, normalize, b.d_cb + build.from * D, b.d_vn2 + build.from,
                              b.d_maxnorm, st), WAX_HIP_ERR_INTERNAL, "mirror kernel launch");
        converted += n_new;
    }
    const std::vector<uint32_t> dirty = fill.take_dirty();    // overwritten since: the listed rows
    hipError_t err = hipSuccess;
    if (!dirty.empty()) {
        err = hipMemcpyAsync(b.d_dirty, dirty.data(), dirty.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
        if (err == hipSuccess) err = hipStreamSynchronize(st);                         // (pageable source: the vector goes next; a rare path)
        if (err == hipSuccess) err = launch_mirror_rows(e->d_store, b.d_dirty, (uint32_t)dirty.size(), D, normalize, b.d_cb, b.d_vn2, b.d_maxnorm, st);
        converted += dirty.size();
    }
    if (err == hipSuccess && converted) err = hipEventRecord(b.ev_ready, st);
    if (err != hipSuccess) {                                  // the list is taken: what it named is converted with everything else
        fill.restart();
        return fail(WAX_HIP_ERR_INTERNAL, std::string("mirror conversion: ") + hipGetErrorString(err));
    }
    if (converted) {
        b.ev_pending = true;
        b.rows_converted += converted;
        b.conversions += 1;
    }
    fill.settle(count);
    return WAX_HIP_OK;
}

// The 8-bit code mirror (mirror8_scan.hip): allocated and built by the query that wants it (search_internal.inc decides when), appended
// rows converted at the next use, anything else converted again as a whole — see BatchMirror. Like ensure_mirror nothing here waits for
// the device: the converting stream records ev8_ready, every other slot's stream waits for it.
int ensure_mirror8(wax_hip_engine* e, hipStream_t st) {
    BatchMirror& b = e->batch;
    RowFill& fill = e->derived.codes;
    std::unique_lock<std::mutex> g(b.mu8);
    if (fill.current() && b.c8_cap >= e->capacity) {
        if (b.ev8_pending) {
            if (hipEventQuery(b.ev8_ready) == hipSuccess) b.ev8_pending = false;
            else HIP_TRY(hipStreamWaitEvent(st, b.ev8_ready, 0), WAX_HIP_ERR_INTERNAL, "code mirror ready wait");
        }
        return WAX_HIP_OK;
    }
    const uint32_t D = e->dims;
    if (!b.d_c8_max) HIP_TRY(hipMalloc(&b.d_c8_max, sizeof(unsigned int)), WAX_HIP_ERR_ALLOC, "Failed to allocate code mirror scalars");
    if (!b.ev8_ready) HIP_TRY(hipEventCreateWithFlags(&b.ev8_ready, hipEventDisableTiming), WAX_HIP_ERR_INTERNAL, "event create");
    if (b.ev8_pending) HIP_TRY(hipStreamWaitEvent(st, b.ev8_ready, 0), WAX_HIP_ERR_INTERNAL, "code mirror ready wait");
    if (b.c8_cap < e->capacity || b.d_c8 == nullptr) {
        // the store was reallocated: as for the bf16 mirror no reader can hold the old buffers (a mutation came first, under the
        // exclusive lock); the codes do not move over, they are converted again
        if (b.ev8_pending) { (void)hipEventSynchronize(b.ev8_ready); b.ev8_pending = false; }
        (void)hipFree(b.d_c8); (void)hipFree(b.d_c8_meta);
        b.d_c8 = nullptr; b.d_c8_meta = nullptr; b.c8_cap = 0;
        fill.restart();
        unsigned char* nc = nullptr; float* nm = nullptr;
        HIP_TRY(hipMalloc(&nc, mirror8_bytes(e->capacity, D)), WAX_HIP_ERR_ALLOC, "Failed to allocate code mirror");   // whole tiles
        if (hipMalloc(&nm, (size_t)e->capacity * 2 * sizeof(float)) != hipSuccess) { (void)hipFree(nc); return fail(WAX_HIP_ERR_ALLOC, "Failed to allocate code mirror row words"); }
        b.d_c8 = nc; b.d_c8_meta = nm; b.c8_cap = e->capacity;
    }
    const uint64_t count = e->count;
    const RowFill::Build build = fill.begin(count);
    if (build.scratch) HIP_TRY(hipMemsetAsync(b.d_c8_max, 0, sizeof(unsigned int), st), WAX_HIP_ERR_INTERNAL, "code mirror memset");
    if (build.from < count) {
        const uint64_t n_new = count - build.from;
        // the bases and the first row: the range may begin inside a tile (mirror8_layout.h)
        const hipError_t err = launch_mirror8_build(e->d_store, build.from, (uint32_t)n_new, D, e->metric == WAX_HIP_METRIC_COSINE ? 1 : 0,
                                                    b.d_c8, b.d_c8_meta, b.d_c8_max, st);
        if (err != hipSuccess) { fill.restart(); return fail(WAX_HIP_ERR_INTERNAL, std::string("code mirror kernel launch: ") + hipGetErrorString(err)); }
        HIP_TRY(hipEventRecord(b.ev8_ready, st), WAX_HIP_ERR_INTERNAL, "code mirror ready record");
        b.ev8_pending = true;
        b.rows8_converted += n_new;
        b.conversions8 += 1;
    }
    fill.settle(count);
    return WAX_HIP_OK;
}

void free_bctx(BatchCtx* c) {
    if (!c) return;
    (void)hipFree(c->d_q); (void)hipFree(c->d_qb); (void)hipFree(c->d_qf); (void)hipFree(c->d_qn2); (void)hipFree(c->d_qnorm); (void)hipFree(c->d_eps);
    (void)hipFree(c->d_tau); (void)hipFree(c->d_dense); (void)hipFree(c->d_cand_count); (void)hipFree(c->d_overflow);
    (void)hipFree(c->d_cand); (void)hipFree(c->d_seg_count); (void)hipFree(c->d_exact); (void)hipFree(c->d_sel);
    (void)hipFree(c->d_tile_max); (void)hipFree(c->d_hits);
    (void)hipHostFree(c->h_hits); (void)hipHostFree(c->h_cert); (void)hipFree(c->d_cert); (void)hipHostFree(c->h_qnorm); (void)hipHostFree(c->h_qlist);
    (void)hipFree(c->d_qlist); (void)hipHostFree(c->h_fnorm); (void)hipFree(c->d_fnorm); (void)hipFree(c->d_mpart); (void)hipFree(c->d_rescue); (void)hipFree(c->d_rescue_exact); (void)hipHostFree(c->h_live);
    if (c->ev_in) (void)hipEventDestroy(c->ev_in);
    if (c->ev_g0) (void)hipEventDestroy(c->ev_g0);
    if (c->ev_g1) (void)hipEventDestroy(c->ev_g1);
    if (c->ev_gc) (void)hipEventDestroy(c->ev_gc);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int alloc_bctx(wax_hip_engine* e, BatchCtx** out) {
    BatchCtx* c = new BatchCtx();
    const uint32_t D = e->dims;
    (void)D;
    hipError_t err = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    auto A = [&](auto** p, size_t bytes) { if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(p), bytes); };
    if (err == hipSuccess) err = hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&c->ev_g0, hipEventReleaseToDevice);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&c->ev_g1, hipEventReleaseToDevice);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&c->ev_gc, hipEventDisableTiming);
    A(&c->d_qb, (size_t)kBatchMaxQ * D * sizeof(unsigned short));
    A(&c->d_qf, (size_t)kBatchMaxQ * D * sizeof(unsigned short));
    A(&c->d_qn2, kBatchMaxQ * sizeof(float));
    A(&c->d_qnorm, kBatchMaxQ * sizeof(float));
    A(&c->d_eps, kBatchMaxQ * sizeof(float));
    A(&c->d_tau, kBatchMaxQ * sizeof(float));
    A(&c->d_cand_count, (size_t)kBatchMaxQ * CAND_COUNT_STRIDE * sizeof(uint32_t));
    A(&c->d_overflow, (kBatchMaxQ + BATCH_PROGRESS_WORDS + BATCH_DYN_WORDS) * sizeof(uint32_t));   // + the filtering GEMM's pace-gate words and tile-claim counters
    A(&c->d_seg_count, (size_t)kBatchMaxSegs * kBatchMaxQ * sizeof(uint32_t));
    A(&c->d_qlist, (size_t)kBatchMaxQ * sizeof(uint32_t));
    A(&c->d_fnorm, (size_t)kBatchMaxQ * sizeof(float));
    if (err == hipSuccess) err = hipHostMalloc(&c->h_qlist, (size_t)kBatchMaxQ * sizeof(uint32_t), hipHostMallocDefault);
    if (err == hipSuccess) err = hipHostMalloc(&c->h_fnorm, (size_t)kBatchMaxQ * sizeof(float), hipHostMallocDefault);
    if (err == hipSuccess) err = hipHostMalloc(&c->h_live, (size_t)kBatchMaxQ * sizeof(uint32_t), hipHostMallocDefault);
    if (err != hipSuccess) {
        free_bctx(c);
        return fail(WAX_HIP_ERR_ALLOC, std::string("Failed to allocate batch workspace: ") + hipGetErrorString(err));
    }
    *out = c;
    return WAX_HIP_OK;
}

constexpr const char* kBatchWorkBusy = "every batch workspace is in use: collect outstanding batch tickets first (or raise \"batch_workspaces\")";

// try_only: the caller holds batch tickets (= workspaces) and is refused where another would wait (work_pool.h). Returned by e->bctxs.release(c).
int take_bctx(wax_hip_engine* e, BatchCtx** out, bool try_only = false) {
    int rc = WAX_HIP_OK;
    const PoolGot got = e->bctxs.acquire(try_only ? PoolMode::tries : PoolMode::wait, out, &rc, [e](int, BatchCtx** made) { return alloc_bctx(e, made); });
    return got == PoolGot::busy ? fail(WAX_HIP_ERR_INVALID_ARGUMENT, kBatchWorkBusy) : rc;
}

// Grow-on-demand buffers of a workspace (idle on its stream when called: a call owns its workspace and starts here).
template <typename T>
int grow_dev(T** p, uint64_t* cap, uint64_t want, size_t elem, const char* what) {
    if (*cap >= want) return WAX_HIP_OK;
    (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(p), (size_t)want * elem), WAX_HIP_ERR_ALLOC, what);
    *cap = want;
    return WAX_HIP_OK;
}

// ---- filtered-search workspaces and the id -> row table ----

void free_filter_work(FilterWork* f) {
    if (!f) return;
    (void)hipFree(f->d_pred_counts); (void)hipFree(f->d_partials); (void)hipFree(f->d_mirror_out);
    if (f->h_pred_counts) (void)hipHostFree(f->h_pred_counts);
    if (f->h_mirror_out) (void)hipHostFree(f->h_mirror_out);
    (void)hipFree(f->d_rows); (void)hipFree(f->d_ids); (void)hipFree(f->d_dist); (void)hipFree(f->d_allow); (void)hipFree(f->d_bitmap);
    (void)hipFree(f->d_block_sum); (void)hipFree(f->d_total); (void)hipFree(f->d_query); (void)hipFree(f->d_qnorm); (void)hipFree(f->d_hits);
    (void)hipFree(f->d_bq); (void)hipFree(f->d_meta); (void)hipFree(f->d_lrows); (void)hipFree(f->d_lcnt); (void)hipFree(f->d_lids);
    (void)hipFree(f->d_part); (void)hipFree(f->d_bhits); (void)hipFree(f->d_tplan); (void)hipFree(f->d_tbits);
    free_select_work(&f->sw);
    if (f->h_total) (void)hipHostFree(f->h_total);
    if (f->h_hits) (void)hipHostFree(f->h_hits);
    if (f->stream) (void)hipStreamDestroy(f->stream);
    delete f;
}

static int alloc_filter_work(wax_hip_engine* e, FilterWork** out) {
    FilterWork* f = new FilterWork();
    struct Guard { FilterWork* f; ~Guard() { if (f) free_filter_work(f); } } guard{f};
    HIP_TRY(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking), WAX_HIP_ERR_INTERNAL, "Failed to create filter stream");
    HIP_TRY(hipMalloc(&f->d_query, (size_t)e->dims * sizeof(float)), WAX_HIP_ERR_ALLOC, "Failed to allocate filter query buffer");
    HIP_TRY(hipMalloc(&f->d_qnorm, sizeof(float)), WAX_HIP_ERR_ALLOC, "Failed to allocate filter scalars");
    HIP_TRY(hipMalloc(&f->d_total, sizeof(uint32_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate filter scalars");
    HIP_TRY(hipHostMalloc(&f->h_total, sizeof(uint32_t), hipHostMallocDefault), WAX_HIP_ERR_ALLOC, "Failed to allocate filter scalars");
    HIP_TRY(hipMalloc(&f->d_hits, (size_t)WAX_HIP_MAX_RESULTS * sizeof(wax_hip_hit)), WAX_HIP_ERR_ALLOC, "Failed to allocate filter hits");
    HIP_TRY(hipHostMalloc(&f->h_hits, (size_t)WAX_HIP_MAX_RESULTS * sizeof(wax_hip_hit), hipHostMallocDefault), WAX_HIP_ERR_ALLOC,
            "Failed to allocate filter hits staging");
    HIP_TRY(alloc_select_work(&f->sw), WAX_HIP_ERR_ALLOC, "Failed to allocate the selection workspace");
    guard.f = nullptr;
    *out = f;
    return WAX_HIP_OK;
}

static int take_filter_work(wax_hip_engine* e, FilterWork** out) {   // waits for one; returned by e->filter_works.release(f)
    int rc = WAX_HIP_OK;
    (void)e->filter_works.acquire(PoolMode::wait, out, &rc, [e](int, FilterWork** made) { return alloc_filter_work(e, made); });
    return rc;
}

// The id -> row table of the store as it is now (shared lock held; pending rows flushed). Concurrent filtered searches
// serialise on the rebuild only.
static int ensure_idhash(wax_hip_engine* e, hipStream_t st) {
    IdHash& h = e->idhash;
    RowFill& fill = e->derived.idtable;
    if (fill.current()) return WAX_HIP_OK;
    std::unique_lock<std::mutex> g(h.mu);
    if (fill.current()) return WAX_HIP_OK;
    uint64_t want = 1024;
    while (want < 2 * e->count) want *= 2;   // load factor <= 0.5
    if (h.slots < want) {
        (void)hipFree(h.d_table);
        h.d_table = nullptr; h.slots = 0;
        fill.restart();
        want *= 2;                                // room for the appends to come: a table that must grow is rebuilt from row 0
        HIP_TRY(hipMalloc(&h.d_table, (size_t)want * sizeof(uint32_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate id table");
        h.slots = want;
    }
    // rows [from, count): all of them after a removal / deserialize / growth (row 0 has the kernel clear the table first), the appended ones otherwise
    const uint64_t from = fill.begin(e->count).from;
    HIP_TRY(launch_idhash_build(e->d_ids, (uint32_t)from, (uint32_t)e->count, h.d_table, h.slots, st), WAX_HIP_ERR_INTERNAL, "id table kernel launch");
    HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "id table build failed on device");
    e->st_idhash_rows += e->count - from;
    fill.settle(e->count);
    return WAX_HIP_OK;
}


// [kBatchMaxQ][kp] scratch of the re-score / large-k' selection (the workspace's stream is idle when this is called)
int bctx_reserve_kp(BatchCtx* c, uint64_t kp) {
    if (c->kp_cap >= kp) return WAX_HIP_OK;
    (void)hipFree(c->d_exact); (void)hipFree(c->d_sel);
    c->d_exact = nullptr; c->d_sel = nullptr; c->kp_cap = 0;
    HIP_TRY(hipMalloc(&c->d_exact, (size_t)kBatchMaxQ * kp * sizeof(int64_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate batch re-score keys");
    HIP_TRY(hipMalloc(&c->d_sel, (size_t)kBatchMaxQ * kp * sizeof(int64_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate batch selection");
    c->kp_cap = kp;
    return WAX_HIP_OK;
}

int bctx_reserve(BatchCtx* c, uint64_t cand_slots, uint64_t kp, uint64_t tile_rows, uint64_t n_queries, bool dense) {
    // [rows of the largest block][cand_slots] keys; capacity tracked in keys
    const uint64_t rows_blk = n_queries < kBatchMaxQ ? ((n_queries + 255ull) & ~255ull) : (uint64_t)kBatchMaxQ;
    int rc = grow_dev(&c->d_cand, &c->cand_slots, rows_blk * cand_slots, sizeof(int64_t), "Failed to allocate batch candidates");
    if (rc != WAX_HIP_OK) return rc;
    rc = bctx_reserve_kp(c, kp);
    if (rc != WAX_HIP_OK) return rc;
    rc = grow_dev(&c->d_tile_max, &c->tile_max_rows, tile_rows, (size_t)kBatchMaxQ * sizeof(float), "Failed to allocate sample maxima");
    if (rc != WAX_HIP_OK) return rc;
    if (dense && !c->d_dense)
        HIP_TRY(hipMalloc(&c->d_dense, (size_t)kBatchMaxQ * kBatchFirstSlab * sizeof(float)), WAX_HIP_ERR_ALLOC, "Failed to allocate first-slab tile");
    if (c->cert_cap < n_queries) {
        uint64_t want = 1024;
        while (want < n_queries) want *= 2;
        (void)hipHostFree(c->h_cert); (void)hipHostFree(c->h_qnorm); (void)hipFree(c->d_cert);
        c->h_cert = nullptr; c->h_qnorm = nullptr; c->d_cert = nullptr; c->cert_cap = 0;
        HIP_TRY(hipHostMalloc(&c->h_cert, want * sizeof(uint32_t), hipHostMallocDefault), WAX_HIP_ERR_ALLOC, "Failed to allocate pinned batch flags");
        HIP_TRY(hipMalloc(&c->d_cert, want * sizeof(uint32_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate batch flags");
        HIP_TRY(hipHostMalloc(&c->h_qnorm, want * sizeof(float), hipHostMallocDefault), WAX_HIP_ERR_ALLOC, "Failed to allocate pinned batch norms");
        c->cert_cap = want;
    }
    return WAX_HIP_OK;
}

// Staging of a host-pointer call: the query block in HBM and the hits on their way back.
int bctx_reserve_host(wax_hip_engine* e, BatchCtx* c, uint64_t nq, uint64_t hits) {
    int rc = grow_dev(&c->d_q, &c->q_cap, nq, (size_t)e->dims * sizeof(float), "Failed to allocate batch queries");
    if (rc != WAX_HIP_OK) return rc;
    if (c->hits_cap < hits) {
        uint64_t want = (uint64_t)kBatchMaxQ * 16;
        while (want < hits) want *= 2;
        (void)hipFree(c->d_hits); (void)hipHostFree(c->h_hits);
        c->d_hits = nullptr; c->h_hits = nullptr; c->hits_cap = 0;
        HIP_TRY(hipMalloc(&c->d_hits, want * sizeof(wax_hip_hit)), WAX_HIP_ERR_ALLOC, "Failed to allocate batch hits");
        HIP_TRY(hipHostMalloc(&c->h_hits, want * sizeof(wax_hip_hit), hipHostMallocDefault), WAX_HIP_ERR_ALLOC, "Failed to allocate pinned batch hits");
        c->hits_cap = want;
    }
    return WAX_HIP_OK;
}

int batch_kp(int k_eff, int kp_max) {
    int kp = 2 * k_eff + 32;
    if (kp < 64) kp = 64;
    if (kp > kp_max) kp = kp_max;
    return kp;
}

// ---- one-pass pipeline: plan -------------------------------------------------------------------------------------
struct OnepassPlan {
    uint32_t tile_rows, ntiles, sample_tiles, rank, seg_area;
    int kp;
    double expect;       // expected survivors per query
};

// tau_sim = the j-th largest of the S sampled tiles' best similarities (pick_tau_kernel). With well-mixed rows the
// number of store rows above it is Gamma(j) / f, f = S * tile_rows / n the sampled fraction: mean j / f, relative spread
// 1 / sqrt(j). The filter fails a query (exact path, ~0.25 ms) when fewer than m ~ 2.2 k rows pass — k for the answer
// plus the rows within the bf16 error band of the k-th — i.e. with probability P(Gamma(j) < m f). The plan takes the
// rank and sample size of least modelled cost among those whose failure probability is below 1e-6 per query (and whose
// expected survivors are at least `batch_survivors` x k', a floor for stores that are not well mixed): survivors cost the filtering GEMM its cold path
// (~10 % of the kernel at 10 k' survivors) and the finish kernel its gather. The minimum of G = 4 group maxima used
// before needed ~10 k' survivors for 1e-5. Sampling costs a tile round (~3 us) per `workgroups per group` tiles and
// visits scattered tiles, so S is held to a few rounds.
constexpr uint32_t kPickJ = 12;      // == PICK_J (batch.hip)
double gamma_cdf_below(uint32_t j, double x) {   // P(Gamma(j, 1) < x) = P(Poisson(x) >= j)
    double term = std::exp(-x), sum = 0.0;
    for (uint32_t i = 1; i <= j + 60; ++i) {
        term *= x / (double)i;               // e^-x x^i / i!
        if (i >= j) sum += term;
    }
    return sum;
}
bool plan_onepass(wax_hip_engine* e, uint32_t n, int k_eff, uint32_t nq, OnepassPlan* p) {
    if (e->batch_onepass.load() == 0 || !batch_onepass_dims(e->dims, e->metric) || k_eff > kBatchMaxK) return false;
    // fast: a register-resident GEMM filters (survivors in per-workgroup segments); otherwise (L2, other multiples of 64)
    // the LDS-tiled kernel does, appending to ONE counted list per query
    const bool fast = batch_onepass_fast(e->dims, e->metric);
    p->tile_rows = batch_tile_rows(e->dims, e->metric);
    p->ntiles = (n + p->tile_rows - 1) / p->tile_rows;
    // too small to sample: slab pipeline ("batch_onepass_tiles" counts units of min(tile rows, 64) rows: 32 at D = 768, 64 elsewhere).
    // Default 64 units since round 6 (1024 before): at 4 096 .. 65 000 rows x 384 a blocking 256-query call takes 95 - 107 us here against
    // 139 - 177 us through the slab pipeline (768-d, 32 and 1 024 queries alike: -30 ... -40 %), and top_k > 80 — which the slab
    // pipeline does not take at all: one scan per query, 8 - 11 ms per 256 queries — 0.25 - 0.37 ms. Below 64 units the sample is
    // half the store and the thresholds admit too much: 2 048 / 3 000 rows 204 us against 107 / 134 (profiles/r06/r_*).
    const uint32_t unit = fast ? std::min<uint32_t>(p->tile_rows, 64u) : 64u;
    if ((int64_t)n < e->batch_onepass_tiles.load() * (int64_t)unit || (fast ? n < 32u * unit : p->ntiles < 512)) return false;
    p->kp = batch_kp(k_eff, 960);
    // k in 81 .. 128: k' = 2k + 32 would need the three-launch finish (select 120-190 us + re-score + finalize at 256 queries on a dense
    // corpus) where the fused finish kernel takes ~58 us. With the device-side retry behind it — which re-scores exactly the survivors the
    // first finish's k-th cannot exclude, whatever k' was — k' = 192 (>= 64 candidates beyond k) loses nothing but a few more retried queries.
    if (e->batch_kp_fused.load() != 0 && p->kp > FUSED_MAX_K && k_eff <= 128 && e->batch_retry.load() == 1 && batch_retry_dims(e->dims))
        p->kp = FUSED_MAX_K;
    const uint32_t nq_blk = nq < kBatchMaxQ ? nq : kBatchMaxQ;
    const uint32_t nq_pad = (nq_blk + 255u) & ~255u;
    const uint32_t groups = nq_pad / BATCH_GROUP_QUERIES;
    uint32_t nseg = fast ? 256 / (groups ? groups : 1) : 1u;   // workgroups per query group == survivor segments per query (1 = counted list)
    if (nseg < 1) nseg = 1;
    if (nseg > p->ntiles) nseg = p->ntiles;
    // sampled tiles that run at once (one "round" ~ 3 us): the persistent workgroups of a query group, or — LDS-tiled kernel,
    // one workgroup per (tile, 128 queries), ~3 resident per CU — 768 workgroups over the batch's query tiles
    const uint32_t samp_par = fast ? nseg : std::max<uint32_t>(1u, 768u / (nq_pad / 128u));
    const double floor_e = (double)e->batch_survivors.load() * (double)p->kp;
    uint64_t s_pref = p->ntiles / (uint64_t)e->batch_sample_div.load();
    if (s_pref < 192) s_pref = 192;
    if (s_pref > 2048) s_pref = 2048;
    if (s_pref > 8ull * samp_par) s_pref = 8ull * samp_par > 192 ? 8ull * samp_par : 192;   // at most 8 tile rounds
    if (s_pref > p->ntiles / 2) s_pref = p->ntiles / 2;
    const double rows = (double)p->tile_rows, nn = (double)n;
    const double need = 2.2 * (double)k_eff;             // rows that must pass: k + those inside the bf16 error band of the k-th
    // Per rank j: the expected survivors E that keep P(Gamma(j) < need * j / E) below 1e-6 (a fallback costs ~0.25 ms: 1e-6 x 1024 queries = 0.3 us per batch), the sample size that gives
    // that E — in general E(j, S) = n (1 - (1 - j/S)^(1/tile_rows)): a fraction j/S of the tiles holds a row above the
    // threshold; ~ j n / (S tile_rows) while j << S, and still a valid (looser) threshold when a small store or a large
    // k forces j close to S — and a cost in microseconds: sampling rounds + cold-path survivors (profiles/r02).
    double best_cost = 0.0;
    p->rank = 0;
    // x_j: P(Gamma(j) < x_j) = 1e-6 — constants (40 bisection steps of a 70-term series each, for eight ranks: ~35 us of host
    // time that used to sit in front of the first launch of EVERY batch; a blocking call paid it in full). Computed once.
    static const std::array<double, kPickJ + 1> kGammaX = [] {
        std::array<double, kPickJ + 1> x{};
        for (uint32_t j = 5; j <= kPickJ; ++j) {
            double lo = 0.0, hi = (double)j;
            for (int it = 0; it < 40; ++it) {
                const double mid = 0.5 * (lo + hi);
                if (gamma_cdf_below(j, mid) > 1e-6) hi = mid; else lo = mid;
            }
            x[j] = lo;
        }
        return x;
    }();
    for (uint32_t j = 5; j <= kPickJ; ++j) {
        const double lo = kGammaX[j];
        double e_need = need * (double)j / lo;
        if (e_need < floor_e) e_need = floor_e;
        if (e_need / nn > 0.25) continue;                 // a quarter of the store as candidates: not a filter any more
        double s_exact = (double)j / (1.0 - std::pow(1.0 - e_need / nn, rows));
        double st = std::floor(s_exact);
        if (st > (double)s_pref) st = (double)s_pref;
        if (st < (double)j + 1.0) st = (double)j + 1.0;
        const double expect = nn * (1.0 - std::pow(1.0 - (double)j / st, 1.0 / rows));
        if (expect / nn > 0.25) continue;
        const double cost = std::ceil(st / (double)samp_par) * 3.0 + expect * 0.031 * 256.0 / (double)(fast ? nseg : 256u);
        if (p->rank == 0 || cost < best_cost) {
            best_cost = cost;
            p->rank = j;
            p->sample_tiles = (uint32_t)st;
            p->expect = expect;
        }
    }
    if (p->rank == 0) return false;
    if (p->expect < 2.0 * (double)k_eff + 8.0) return false;   // cannot reach enough candidates for the certificate: other paths
    // Survivor segments: one per (GEMM workgroup of the query's group, query). A query's survivor count spreads around
    // `expect` like Gamma(rank) (x 2.3 at 1e-4 for rank 12; clustered stores spread more), and a segment overflows when
    // ITS fill does: size every segment for 4 x expect spread over the group's workgroups, + 6 sigma of a Poisson fill
    // (an overflow only costs that query the exact path, but at 0.25 ms each two of them per batch doubled the batch
    // time: profiles/r02/c_onepass_diag.txt).
    // ... and at least 128 slots per segment (8 192 for the one counted list): memory is not the constraint (32 K keys per
    // query = 64 MB for a 256-query block), and a run of near-duplicate rows — consecutive chunks of one document — lands in
    // the few segments whose workgroups own those tiles: 64 survivors from one 64-row tile, not the ~1 of well-mixed rows.
    // Roomy segments are what lets the full retry (re-score every survivor) answer such queries without a pass over the store.
    const double fill = 4.0 * p->expect / (double)nseg;
    uint64_t slots = fast ? 128 : 8192;
    while ((double)slots < fill + 6.0 * std::sqrt(fill) + 4.0) slots *= 2;
    const uint64_t area = slots * nseg;
    if (area > 262144) return false;
    p->seg_area = (uint32_t)area;
    return true;
}

// Enqueue the whole batch pipeline for <= kBatchMaxQ device-resident queries on the workspace's stream: hits land in
// d_out[q * out_stride .. + out_stride) (k_eff real entries, the rest padded), certificate flags in ctx->h_cert +
// cert_off, exact norms in ctx->h_qnorm + cert_off (pinned host memory the kernels write directly). Nothing is synchronised here.
int batch_enqueue(wax_hip_engine* e, BatchCtx* c, const float* d_queries, uint32_t qn, int k_eff, const OnepassPlan* plan,
                  wax_hip_hit* d_out, uint32_t out_stride, uint32_t cert_off) {
    BatchMirror& b = e->batch;
    hipStream_t st = c->stream;
    const uint32_t D = e->dims;
    const uint32_t n = (uint32_t)e->count;
    const uint32_t nq_pad = (qn + 255u) & ~255u;  // 256: the register-resident-queries GEMM works on groups of 256
    PrepArgs pa{};
    pa.queries = d_queries; pa.nq = qn; pa.nq_pad = nq_pad; pa.dims = D; pa.metric = e->metric;
    pa.max_bits = b.d_maxnorm;                                   // {max ||v||, max ||x - bf16(x)||} as the mirror's conversions left them, read on the device
    pa.use_measured = e->batch_eps_measured.load() != 0 ? 1 : 0;
    const bool frag_order = e->batch_qfrag.load() != 0 && (D % 16u) == 0;   // "batch_qfrag" (default 1): fragment-ordered query copy for the rq GEMM
    pa.qf = frag_order ? c->d_qf : nullptr;
    pa.qb = c->d_qb; pa.q_n2 = c->d_qn2; pa.q_norm = c->d_qnorm; pa.eps = c->d_eps; pa.tau = c->d_tau; pa.overflow = c->d_overflow;
    const bool counted = plan != nullptr && !batch_onepass_fast(D, e->metric);   // one-pass on the LDS-tiled kernel: one counted list per query
    pa.cand_count = (plan && !counted) ? nullptr : c->d_cand_count;
    pa.q_norm_host = c->h_qnorm + cert_off;
    // the words behind the overflow flags: the progress words of the 768-d filtering GEMM's pace gate — zeroed by the prep kernel
    const bool pace_gate = plan != nullptr && D == 768 && nq_pad > 256;
    pa.progress = pace_gate ? c->d_overflow + kBatchMaxQ : nullptr;
    // and behind those the claim counters of its tail pool ("batch_dyn_tail", default 1) — zeroed by the prep kernel too
    static_assert(kBatchMaxQ / 256 * 32 <= BATCH_DYN_WORDS, "one 128-byte line of claim counters per query group");
    pa.dyn = (plan != nullptr && e->batch_dyn_tail.load() != 0) ? c->d_overflow + kBatchMaxQ + BATCH_PROGRESS_WORDS : nullptr;
    HIP_TRY(launch_batch_prep(pa, st), WAX_HIP_ERR_INTERNAL, "batch prep launch");
    GemmArgs g{};
    g.qf = frag_order ? c->d_qf : nullptr;
    g.qb = c->d_qb; g.cb = b.d_cb; g.q_n2 = c->d_qn2; g.v_n2 = b.d_vn2; g.tau = c->d_tau;
    g.cand = c->d_cand; g.cand_count = c->d_cand_count; g.row_base = (uint32_t)e->row_base;
    g.dims = D; g.n_rows = n; g.nq = qn; g.nqt = nq_pad / 128;
    g.use_rega = (uint32_t)e->batch_rega.load();  // 0 LDS-tiled kernel, 1 workgroup barrier per tile (default), 5 split barrier
    g.debug = (uint32_t)e->batch_debug.load();
    g.prof = reinterpret_cast<uint32_t*>((uintptr_t)e->batch_prof_ptr.load());
    g.seg_count = c->d_seg_count;
    if (plan) {
        // ---- one pass: sample -> threshold -> filter everything -> finish ----
        g.slab0 = 0; g.slab_rows = n; g.dense = nullptr; g.dense_ld = 0;
        g.cand_cap = plan->seg_area; g.seg_base = 0; g.seg_area = plan->seg_area;
        if (g.use_rega == 0) g.use_rega = 1;
        GemmArgs gs = g;
        gs.tile_max = c->d_tile_max; gs.sample_tiles = plan->sample_tiles;
        g.progress = pa.progress;
        g.dyn = pa.dyn;
        HIP_TRY(launch_batch_gemm_sample(gs, e->metric, st), WAX_HIP_ERR_INTERNAL, "sampling gemm launch");
        const int tk_mode = (int)e->time_kernels.load();   // read once per batch
        const bool timed = tk_mode != 0;
        std::unique_lock<std::mutex> cg(e->gemm_chain_mu, std::defer_lock);
        if (timed) {
            // (the chain wait sits in front of the threshold kernel: the sampling GEMM before it could not get a CU
            // until the previous batch's filtering GEMM left anyway, and one packet less separates threshold and GEMM)
            cg.lock();
            if (e->gemm_chain_ev && e->gemm_chain_ev != c->ev_g1 && e->gemm_chain_ev != c->ev_gc)
                HIP_TRY(hipStreamWaitEvent(st, e->gemm_chain_ev, 0), WAX_HIP_ERR_INTERNAL, "gemm chain wait");
        }
        HIP_TRY(launch_pick_tau(c->d_tile_max, plan->sample_tiles, qn, nq_pad, plan->rank, c->d_tau, e->metric, st), WAX_HIP_ERR_INTERNAL,
                "threshold kernel launch");
        if (timed) {
            // With several batches in flight (submit / collect) the filtering GEMMs of different workspaces would queue
            // for the same CUs (one workgroup's LDS fills a CU) and an event interval would include that wait: chain
            // them, like the single-query scans, so that a timed interval is one GEMM running alone. The small
            // kernels before this point (prep, sampling, thresholds) still overlap the previous batch's GEMM tail
            // and finish kernel.
            if (tk_mode == 2) {
                // kernel-bound pair (kernels.h: launch_kernel)
                launch_timing() = LaunchTiming{c->ev_g0, c->ev_g1};
                const hipError_t lerr = launch_batch_gemm(g, e->metric, st);
                launch_timing() = LaunchTiming{};
                HIP_TRY(lerr, WAX_HIP_ERR_INTERNAL, "gemm kernel launch");
                HIP_TRY(hipEventRecord(c->ev_gc, st), WAX_HIP_ERR_INTERNAL, "event record");
                e->gemm_chain_ev = c->ev_gc;
            } else {
                HIP_TRY(hipEventRecord(c->ev_g0, st), WAX_HIP_ERR_INTERNAL, "event record");
                HIP_TRY(launch_batch_gemm(g, e->metric, st), WAX_HIP_ERR_INTERNAL, "gemm kernel launch");
                HIP_TRY(hipEventRecord(c->ev_g1, st), WAX_HIP_ERR_INTERNAL, "event record");
                e->gemm_chain_ev = c->ev_g1;
            }
            c->gemm_timed = true; c->gemm_rows = n; c->gemm_queries = qn;
        } else {
            HIP_TRY(launch_batch_gemm(g, e->metric, st), WAX_HIP_ERR_INTERNAL, "gemm kernel launch");
        }
        FinishArgs f{};
        f.cand = c->d_cand; f.cand_cap = plan->seg_area; f.seg_count = c->d_seg_count; f.nq_pad = nq_pad;
        if (counted) {
            f.nseg = 1; f.seg_slots = plan->seg_area; f.seg_count = c->d_cand_count; f.count_stride = CAND_COUNT_STRIDE;
        } else if (!batch_gemm_segments(g, e->metric, &f.nseg, &f.seg_slots)) {
            return fail(WAX_HIP_ERR_INTERNAL, "one-pass plan without a segment kernel");
        }
        f.tau = c->d_tau; f.overflow = c->d_overflow; f.store = e->d_store; f.queries = d_queries; f.q_norm = c->d_qnorm;
        f.eps = c->d_eps; f.ids = e->d_ids; f.n_rows = n; f.row_base = (uint32_t)e->row_base; f.dims = D; f.nq = qn;
        f.kp = plan->kp; f.k = k_eff; f.sel = c->d_sel; f.exact = c->d_exact; f.out = d_out; f.out_stride = out_stride;
        f.certified = c->h_cert + cert_off;   // pinned host memory, written by the kernel: no copy launch behind the finish kernel
        f.cert_dev = c->d_cert + cert_off;
        f.retry_all = (e->batch_debug.load() & 65536) != 0 ? 1u : 0u;
        HIP_TRY(launch_batch_finish(f, e->metric, st), WAX_HIP_ERR_INTERNAL, "finish kernel launch");
        // "batch_retry" 1 (default): while recent batches had queries the first finish could not certify (`retry_hint`, set at
        // collect), the device-side full retry rides behind the finish kernel — uncertified queries get ALL their survivors
        // re-scored without a host round trip; certified ones cost their workgroup one flag read. A store whose batches certify
        // never pays for the launch. 2: the host-driven full retry of round 3 only; 0: neither (exact path at once).
        if (e->batch_retry.load() == 1 && e->retry_hint.load() > 0 && k_eff <= FUSED_MAX_K && batch_retry_dims(D) && !counted)
            HIP_TRY(launch_batch_retry(f, e->metric, st), WAX_HIP_ERR_INTERNAL, "retry kernel launch");
        c->last_finish = f; c->last_metric = e->metric;
        c->last_finish_valid = cert_off == 0;   // the candidate segments survive until collect only for a one-block batch
        e->st_onepass_queries += qn;
    } else {
        // ---- slab pipeline (small stores, L2, other dims): thresholds tightened between geometrically growing slabs ----
        c->last_finish_valid = false;
        const int kp = batch_kp(k_eff, FUSED_MAX_K);
        uint64_t max_slab = (uint64_t)e->batch_slab_mb.load() * 16384ull;  // "slab_mb" MB of f32 scores per 256 queries
        if (max_slab < 2048) max_slab = 2048;
        g.cand_cap = kBatchCandCap; g.seg_base = kBatchSegBase; g.seg_area = kBatchSegArea; g.dense_ld = kBatchFirstSlab;
        // Slabs grow geometrically: with tau tightened after each slab, a slab of s rows appends about
        // kp * s / rows_seen candidates per query, so "next slab = growth x rows seen" keeps every list ~growth*kp long.
        uint32_t s0 = 0;
        while (s0 < n) {
            uint64_t want = (s0 == 0) ? (uint64_t)e->batch_first.load() : (uint64_t)e->batch_growth.load() * s0;
            if (want > max_slab) want = max_slab;
            want = (want + 127ull) & ~127ull;
            const uint32_t rows = (n - s0 < want) ? n - s0 : (uint32_t)want;
            const bool first = (s0 == 0);  // no threshold yet: dense tile instead of appending everything
            g.slab0 = s0; g.slab_rows = rows; g.dense = first ? c->d_dense : nullptr;
            HIP_TRY(launch_batch_gemm(g, e->metric, st), WAX_HIP_ERR_INTERNAL, "gemm kernel launch");
            TightenArgs t{};
            t.cand = c->d_cand; t.cand_cap = kBatchCandCap; t.cand_count = c->d_cand_count; t.kp = kp; t.nq = qn;
            t.tau = c->d_tau; t.overflow = c->d_overflow;
            t.dense = first ? c->d_dense : nullptr; t.dense_ld = kBatchFirstSlab; t.dense_rows = rows;
            t.dense_row0 = (uint32_t)e->row_base + s0;
            t.seg_count = c->d_seg_count; t.seg_base = kBatchSegBase; t.nq_pad = nq_pad;
            if (!batch_gemm_segments(g, e->metric, &t.nseg, &t.seg_slots)) { t.nseg = 0; t.seg_slots = 0; }
            HIP_TRY(launch_tighten(t, st), WAX_HIP_ERR_INTERNAL, "tighten kernel launch");
            s0 += rows;
        }
        RescoreArgs r{};
        r.store = e->d_store; r.queries = d_queries; r.q_norm = c->d_qnorm; r.cand = c->d_cand; r.exact = c->d_exact;
        r.n_rows = n; r.row_base = (uint32_t)e->row_base; r.dims = D; r.nq = qn; r.cand_cap = kBatchCandCap; r.kp = kp;
        HIP_TRY(launch_rescore(r, e->metric, st), WAX_HIP_ERR_INTERNAL, "rescore kernel launch");
        HIP_TRY(launch_finalize_batch(c->d_cand, kBatchCandCap, c->d_overflow, c->d_exact, kp, k_eff, c->d_eps, e->d_ids,
                                      (uint32_t)e->row_base, n, qn, d_out, out_stride, c->h_cert + cert_off, st),
                WAX_HIP_ERR_INTERNAL, "finalize kernel launch");
    }
    e->st_batch_queries += qn;
    e->st_searches += qn;
    e->st_rows += (uint64_t)qn * n;
    e->st_bytes += (uint64_t)n * D * 2ull;
    return WAX_HIP_OK;
}

// Can the MFMA pipelines answer (nq queries, k_eff) on this engine at all?
bool batch_mfma_applicable(wax_hip_engine* e, uint32_t dims, int k_eff, uint32_t nq, OnepassPlan* plan, bool* onepass) {
    if (e->batch_mode.load() == 0 || dims != e->dims || (dims % 64u) != 0 || e->count == 0 || k_eff <= 0) return false;
    *onepass = plan_onepass(e, (uint32_t)e->count, k_eff, nq, plan);
    return *onepass || k_eff <= kBatchMaxKSlab;
}

// The whole batched search on device-resident queries (shared lock held, mirror ready): enqueue every block of
// kBatchMaxQ queries back to back (no host round trip in between), one synchronisation, then the uncertified queries are
// re-run on the exact single-query path, their hits written over the same rows of d_out. d_out rows are out_stride wide.
// Enqueue a whole device-resident batch (blocks of <= kBatchMaxQ queries) on the workspace's stream, followed by the
// download of the certificate flags and exact norms. Nothing is synchronised: batch_finish_device_locked completes it.
int batch_submit_device_locked(wax_hip_engine* e, BatchCtx* c, const float* d_queries, uint32_t nq, int k_eff,
                               const OnepassPlan* plan, wax_hip_hit* d_out, uint32_t out_stride) {
    hipStream_t st = c->stream;
    const uint32_t D = e->dims;
    int rc = bctx_reserve(c, plan ? plan->seg_area : kBatchCandCap, plan ? (uint64_t)plan->kp : (uint64_t)FUSED_MAX_K,
                          plan ? plan->sample_tiles : 0, nq, plan == nullptr);
    if (rc != WAX_HIP_OK) return rc;
    for (uint32_t q0 = 0; q0 < nq; q0 += kBatchMaxQ) {
        const uint32_t qn = (nq - q0 < kBatchMaxQ) ? nq - q0 : kBatchMaxQ;
        rc = batch_enqueue(e, c, d_queries + (uint64_t)q0 * D, qn, k_eff, plan, d_out + (uint64_t)q0 * out_stride, out_stride, q0);
        if (rc != WAX_HIP_OK) { (void)hipStreamSynchronize(st); return rc; }
    }
    // certificate flags and exact norms are written by the kernels straight into pinned host memory (h_cert, h_qnorm)
    return WAX_HIP_OK;
}

// Exact answers for `nf` queries of a device-resident block (rows fq[i] of d_queries, norms h_norm_by_query[fq[i]]), hits
// into rows fq[i] of d_out, on the workspace's stream; synchronised on return. Groups of scan_multi_group() queries share
// one pass over the f32 store; what the multi-query kernel does not serve (k > 192, unspecialised dims, a single query)
// takes one fused / general scan per query as before.
int exact_scan_queries(wax_hip_engine* e, BatchCtx* c, const float* d_queries, const uint32_t* fq, const float* h_norm_by_query,
                       uint32_t nf, int k_eff, wax_hip_hit* d_out, uint32_t out_stride) {
    hipStream_t st = c->stream;
    const uint32_t D = e->dims;
    const uint32_t n = (uint32_t)e->count;
    int rc = WAX_HIP_OK;
    uint32_t done = 0;
    const uint32_t group = (e->batch_multi.load() != 0 && nf >= 2 && e->force_general.load() == 0) ? scan_multi_group(D, k_eff) : 0u;
    if (group >= 2) {
        const int grid = scan_multi_grid(n, D, (int)e->grid_blocks.load());
        rc = grow_dev(&c->d_mpart, &c->mpart_cap, (uint64_t)group * (uint64_t)grid * (uint64_t)k_eff, sizeof(int64_t),
                      "Failed to allocate exact-pass partials");
        if (rc != WAX_HIP_OK) return rc;
        for (uint32_t base = 0; base < nf && rc == WAX_HIP_OK; base += kBatchMaxQ) {
            const uint32_t m = nf - base < kBatchMaxQ ? nf - base : kBatchMaxQ;
            for (uint32_t i = 0; i < m; ++i) {
                c->h_qlist[i] = fq[base + i];
                c->h_fnorm[i] = h_norm_by_query[fq[base + i]];
            }
            HIP_TRY(hipMemcpyAsync(c->d_qlist, c->h_qlist, m * sizeof(uint32_t), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "exact-pass list upload");
            HIP_TRY(hipMemcpyAsync(c->d_fnorm, c->h_fnorm, m * sizeof(float), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "exact-pass norm upload");
            for (uint32_t g0 = 0; g0 < m; g0 += group) {
                ScanMultiArgs a{};
                a.store = e->d_store; a.queries = d_queries; a.qlist = c->d_qlist + g0; a.q_norm = c->d_fnorm + g0;
                a.partials = c->d_mpart; a.n_rows = n; a.row_base = (uint32_t)e->row_base; a.dims = D;
                a.nq = m - g0 < group ? m - g0 : group; a.k = k_eff;
                int used_grid = 0;
                HIP_TRY(launch_scan_multi(a, e->metric, (int)e->grid_blocks.load(), st, &used_grid), WAX_HIP_ERR_INTERNAL, "multi-query scan launch");
                HIP_TRY(launch_merge_keys_multi(c->d_mpart, (uint32_t)used_grid, k_eff, e->d_ids, a.row_base, n, d_out, out_stride,
                                                c->d_qlist + g0, a.nq, st), WAX_HIP_ERR_INTERNAL, "multi-query merge launch");
                e->st_multi_passes += 1;
                e->st_rows += e->count;
                e->st_bytes += e->count * (uint64_t)D * 4ull;
            }
            HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "exact pass failed on device");   // the pinned lists are reused
            done += m;
        }
        e->st_multi_queries += done;
        e->st_searches += done;
        return rc;
    }
    Slot* s = nullptr;
    for (; done < nf; ++done) {
        const uint32_t q = fq[done];
        if (!s) {
            rc = take_slot(e, &s, /*try_only=*/false, /*holder=*/true);
            if (rc != WAX_HIP_OK) return rc;
        }
        rc = enqueue_scan(e, d_queries + (uint64_t)q * D, h_norm_by_query[q], k_eff, (int)out_stride, s->d_partials, s,
                          d_out + (uint64_t)q * out_stride, st, nullptr, nullptr, /*chain=*/false);
        if (rc != WAX_HIP_OK) break;
    }
    if (s) {
        (void)hipStreamSynchronize(st);
        e->slots.release(s);
    }
    return rc;
}

// Wait for a submitted batch; queries whose certificate failed (ties, clustered data, an overflowed list) are answered
// by the exact path in place — never an approximation.
// out_rewritten: queries whose rows of d_out were written HERE (full retries + exact path), i.e. after whatever the caller
// enqueued behind the submit — the sharded handle re-sends a shard's part when it is not 0.
int batch_finish_device_locked(wax_hip_engine* e, BatchCtx* c, const float* d_queries, uint32_t nq, int k_eff,
                               wax_hip_hit* d_out, uint32_t out_stride, uint32_t* out_fallbacks, uint32_t* out_rewritten = nullptr) {
    uint32_t retried = 0;
    hipStream_t st = c->stream;
    const uint32_t D = e->dims;
    HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "batch search failed on device");
    if (c->gemm_timed) {
        c->gemm_timed = false;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev_g0, c->ev_g1) == hipSuccess) {
            std::unique_lock<std::mutex> sg(e->st_mu);
            e->st_gemm_ms += ms; e->st_gemm_timed += 1; e->st_gemm_rows += c->gemm_rows; e->st_gemm_queries += c->gemm_queries;
        }
    }
    int rc = WAX_HIP_OK;
    {   // queries the device-side full retry certified (flag value 2); and the hint that decides whether the NEXT batches carry
        // the retry kernel: armed (for 16 batches) by any query the first finish left uncertified, counted down by clean batches
        uint32_t inl = 0, unc = 0;
        for (uint32_t q = 0; q < nq; ++q) { inl += c->h_cert[q] == 2u; unc += c->h_cert[q] != 1u; }
        e->st_batch_retries += inl;
        e->st_batch_inline_retries += inl;
        if (unc > 0) e->retry_hint.store(16);
        else {   // count a clean batch down, never below zero (concurrent collects race on this word)
            int cur = e->retry_hint.load();
            while (cur > 0 && !e->retry_hint.compare_exchange_weak(cur, cur - 1)) {}
        }
    }
    // Second rung of the ladder, without another pass over the store: an uncertified query's survivors — EVERY row the
    // filtering GEMM admitted (approx distance <= tau) — are still in its segments, so all of them are re-scored exactly
    // (rescore_kernel in survivor-area mode) and the best k selected (full_retry_select_kernel). With every survivor re-scored
    // the certificate only needs tau - eps > the exact k-th: it no longer matters how many rows sit inside the bf16 error band
    // of the k-th neighbour (dense neighbourhoods, runs of near-duplicates: what k' = 2k + 32 candidates cannot cover), only
    // that no segment overflowed — which is why the planner gives every segment room for 128 survivors. A query that fails
    // again (overflow, fewer than k survivors, a tie ACROSS the threshold) goes to the exact path below.
    if (c->last_finish_valid && nq <= kBatchMaxQ && e->batch_retry.load() != 0 && batch_finish_fused_dims(D)) {
        std::vector<uint32_t> failing;
        for (uint32_t q = 0; q < nq; ++q)
            if (!c->h_cert[q]) failing.push_back(q);
        const FinishArgs& lf = c->last_finish;
        const uint64_t area = lf.cand_cap;
        const uint64_t per_round = std::max<uint64_t>(1, std::min<uint64_t>(kBatchMaxQ, (64ull << 20) / (area * sizeof(int64_t))));
        for (size_t off = 0; off < failing.size() && rc == WAX_HIP_OK; off += per_round) {
            const uint32_t m = (uint32_t)std::min<uint64_t>(per_round, failing.size() - off);
            rc = grow_dev(&c->d_rescue, &c->rescue_cap, (uint64_t)m * area, sizeof(int64_t), "Failed to allocate full-retry keys");
            if (rc != WAX_HIP_OK) { rc = WAX_HIP_OK; break; }   // no memory for the retry: the exact path still answers
            std::memcpy(c->h_qlist, failing.data() + off, m * sizeof(uint32_t));
            HIP_TRY(hipMemcpyAsync(c->d_qlist, c->h_qlist, m * sizeof(uint32_t), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "retry list upload");
            // step 1: the live survivors of every query of the round, packed; their counts come back through pinned memory
            CompactArgs ca{};
            ca.cand = lf.cand; ca.cand_cap = lf.cand_cap; ca.seg_count = lf.seg_count; ca.nseg = lf.nseg; ca.seg_slots = lf.seg_slots;
            ca.nq_pad = lf.nq_pad; ca.count_stride = lf.count_stride; ca.qlist = c->d_qlist; ca.n_slots = m;
            ca.dense = c->d_rescue; ca.dense_stride = (uint32_t)area; ca.live_out = c->h_live;
            HIP_TRY(launch_compact_survivors(ca, st), WAX_HIP_ERR_INTERNAL, "full-retry compaction launch");
            HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "full retry failed on device");
            uint32_t live_max = 0;
            for (uint32_t i = 0; i < m; ++i) live_max = std::max(live_max, c->h_live[i]);
            if (live_max == 0) continue;                      // nothing passed the filter: the exact path answers
            const uint32_t kp = (uint32_t)std::min<uint64_t>(area, ((uint64_t)live_max + 63u) & ~63ull);
            rc = grow_dev(&c->d_rescue_exact, &c->rescue_exact_cap, (uint64_t)m * kp, sizeof(int64_t), "Failed to allocate full-retry keys");
            if (rc != WAX_HIP_OK) { rc = WAX_HIP_OK; break; }
            // step 2: exact f32 distance of every survivor (scan_kernel's arithmetic)
            RescoreArgs r{};
            r.store = e->d_store; r.queries = d_queries; r.q_norm = c->d_qnorm; r.cand = c->d_rescue; r.exact = c->d_rescue_exact;
            r.n_rows = lf.n_rows; r.row_base = lf.row_base; r.dims = D; r.nq = m; r.cand_cap = (uint32_t)area; r.kp = (int)kp;
            r.qlist = c->d_qlist; r.by_slot = 1;
            HIP_TRY(launch_rescore(r, c->last_metric, st), WAX_HIP_ERR_INTERNAL, "full-retry rescore launch");
            // step 3: the k best + certificate
            FullRetryArgs fr{};
            fr.exact = c->d_rescue_exact; fr.area = kp; fr.qlist = c->d_qlist; fr.n_slots = m;
            fr.seg_count = lf.seg_count; fr.nseg = lf.nseg; fr.seg_slots = lf.seg_slots; fr.nq_pad = lf.nq_pad; fr.count_stride = lf.count_stride;
            fr.tau = lf.tau; fr.eps = lf.eps; fr.overflow = lf.overflow; fr.ids = lf.ids; fr.n_rows = lf.n_rows; fr.row_base = lf.row_base;
            fr.k = lf.k; fr.out = lf.out; fr.out_stride = lf.out_stride; fr.certified = lf.certified;
            HIP_TRY(launch_full_retry_select(fr, st), WAX_HIP_ERR_INTERNAL, "full-retry select launch");
            HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "full retry failed on device");   // the pinned list is reused; flags are read below
            e->st_batch_retries += m;
            retried += m;
        }
    }
    c->last_finish_valid = false;
    // Exact path for whatever is still uncertified. The queries share passes over the f32 store (up to 16 per pass,
    // scan_multi_kernel: scan_kernel's arithmetic, bit-identical distances) instead of taking one scan each.
    std::vector<uint32_t> failed;
    for (uint32_t q = 0; q < nq; ++q)
        if (!c->h_cert[q]) failed.push_back(q);
    const uint32_t fallbacks = (uint32_t)failed.size();
    if (fallbacks > 0) rc = exact_scan_queries(e, c, d_queries, failed.data(), c->h_qnorm, fallbacks, k_eff, d_out, out_stride);
    e->st_batch_fallbacks += fallbacks;
    if (out_fallbacks) *out_fallbacks = fallbacks;
    if (out_rewritten) *out_rewritten = retried + fallbacks;
    return rc;
}

int batch_search_device_locked(wax_hip_engine* e, BatchCtx* c, const float* d_queries, uint32_t nq, int k_eff,
                               const OnepassPlan* plan, wax_hip_hit* d_out, uint32_t out_stride, uint32_t* out_fallbacks) {
    int rc = batch_submit_device_locked(e, c, d_queries, nq, k_eff, plan, d_out, out_stride);
    if (rc != WAX_HIP_OK) return rc;
    return batch_finish_device_locked(e, c, d_queries, nq, k_eff, d_out, out_stride, out_fallbacks);
}

// "MV2V" encoding-2 segment: header + lengths, in MetalVectorEngine.deserialize's validation order and with its reasons
// (:716-808). One copy for the single-device engine and the sharded handle.
int validate_mv2v_segment(uint8_t metric, uint32_t engine_dims, const uint8_t* data, size_t len, uint64_t* out_n, uint64_t* out_vec_len,
                          uint64_t* out_id_len) {
    if (len < 36) return fail(WAX_HIP_ERR_BAD_SEGMENT, "Metal segment too small: " + std::to_string(len) + " bytes");
    const uint8_t magic[4] = {0x4D, 0x56, 0x32, 0x56};
    if (std::memcmp(data, magic, 4) != 0) return fail(WAX_HIP_ERR_BAD_SEGMENT, "Metal segment magic mismatch");
    uint16_t ver; std::memcpy(&ver, data + 4, 2);
    if (ver != 1) return fail(WAX_HIP_ERR_BAD_SEGMENT, "Unsupported Metal segment version " + std::to_string(ver));
    if (data[6] != 2) return fail(WAX_HIP_ERR_BAD_SEGMENT, "Unsupported Metal segment encoding " + std::to_string((int)data[6]));
    if (data[7] > 2 || data[7] != metric)
        return fail(WAX_HIP_ERR_BAD_SEGMENT, "Metric mismatch: expected " + std::to_string((int)metric) + ", got " + std::to_string((int)data[7]));
    uint32_t dims; std::memcpy(&dims, data + 8, 4);
    if (dims != engine_dims) return fail(WAX_HIP_ERR_BAD_SEGMENT, "Dimension mismatch: expected " + std::to_string(engine_dims) + ", got " + std::to_string(dims));
    uint64_t n, vec_len; std::memcpy(&n, data + 12, 8); std::memcpy(&vec_len, data + 20, 8);
    for (int i = 0; i < 8; ++i)
        if (data[28 + i] != 0) return fail(WAX_HIP_ERR_BAD_SEGMENT, "Metal segment reserved bytes must be zero");
    if (n > 0xffffffffull || vec_len != n * (uint64_t)dims * 4ull) return fail(WAX_HIP_ERR_BAD_SEGMENT, "Vector data length mismatch");
    if ((uint64_t)len < 36 + vec_len + 8) return fail(WAX_HIP_ERR_BAD_SEGMENT, "Metal segment missing frameId length");
    uint64_t id_len; std::memcpy(&id_len, data + 36 + vec_len, 8);
    if (id_len != n * 8ull) return fail(WAX_HIP_ERR_BAD_SEGMENT, "FrameId data length mismatch");
    if ((uint64_t)len < 36 + vec_len + 8 + id_len) return fail(WAX_HIP_ERR_BAD_SEGMENT, "Metal segment truncated frameId data");
    *out_n = n; *out_vec_len = vec_len; *out_id_len = id_len;
    return WAX_HIP_OK;
}

bool device_is_gfx950(int dev) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) != hipSuccess) return false;
    return std::strncmp(p.gcnArchName, "gfx950", 6) == 0;
}

}  // namespace

