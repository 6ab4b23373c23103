// api_timeline.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: the timeline lane (Wax.timeline, TimelineQuery.swift:38-53; UnifiedSearch.swift:181-194) — the `limit` newest or oldest rows
// that pass a row predicate, selected on the device from the attribute columns by the pair (timestamp, frame id) (timeline.hip;
// DESIGN 4.9): the blocking form, the device form on a caller's stream, and a stateless probe of the two kernels.

static void timeline_args(TimelineArgs* a, const wax_hip_row_predicate* pred, int32_t limit, int newest_first) {
    const wax_hip_row_predicate p = normalised_predicate(pred);
    *a = TimelineArgs{};
    a->limit = limit; a->newest = newest_first != 0 ? 1 : 0;
    a->has_after = p.has_after; a->has_before = p.has_before; a->after = p.after; a->before = p.before; a->deny_flags = p.deny_flags;
}

static int timeline_refuse_limit(int32_t limit) {
    if (limit > WAX_HIP_TIMELINE_MAX_LIMIT) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "timeline: limit exceeds WAX_HIP_TIMELINE_MAX_LIMIT (4096)");
    return WAX_HIP_OK;
}

int wax_hip_timeline(wax_hip_engine* e, int32_t limit, int newest_first, const wax_hip_row_predicate* pred, uint64_t* out_ids,
                     int64_t* out_timestamps, uint32_t out_capacity, uint32_t* out_count) {
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (!out_count || (!out_ids && out_capacity)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    { const int lrc = timeline_refuse_limit(limit); if (lrc != WAX_HIP_OK) return lrc; }
    *out_count = 0;
    if (limit <= 0) return WAX_HIP_OK;                          // TimelineQuery.swift:51
    if (e->sh) return sh_timeline(e, limit, newest_first, pred, out_ids, out_timestamps, out_capacity, out_count);
    const int32_t want = (uint32_t)limit < out_capacity ? limit : (int32_t)out_capacity;   // a prefix of the prefix
    if (want == 0) return WAX_HIP_OK;
    DeviceGuard g(e->device);
    ReadGuard rd(e);
    { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return frc; }
    if (e->count == 0) return WAX_HIP_OK;
    FilterLease lease(e);
    if (lease.rc != WAX_HIP_OK) return lease.rc;
    FilterWork& f = lease.work();
    hipStream_t st = f.stream;
    TimelineArgs a;
    timeline_args(&a, pred, want, newest_first);
    { const int arc = ensure_attrs(e, st, &a.ts, &a.flags); if (arc != WAX_HIP_OK) return arc; }
    a.ids = e->d_ids; a.n_rows = e->count;
    const uint32_t grid = timeline_grid(e->count, want);
    const uint64_t scratch = timeline_scratch_words(grid, want), out_words = 2ull * (uint64_t)want + 1ull;
    { const int grc = grow_dev(&f.d_part, &f.part_cap, scratch + out_words, sizeof(int64_t), "Failed to allocate timeline partials"); if (grc != WAX_HIP_OK) return grc; }
    int64_t* d_out = f.d_part + scratch;                         // [want] ids, [want] timestamps, the count
    a.out_ids = reinterpret_cast<uint64_t*>(d_out); a.out_ts = d_out + want; a.out_count = reinterpret_cast<uint32_t*>(d_out + 2 * (size_t)want);
    static_assert((2ull * WAX_HIP_TIMELINE_MAX_LIMIT + 1ull) * sizeof(int64_t) <= (size_t)WAX_HIP_MAX_RESULTS * sizeof(wax_hip_hit), "the pinned hit buffer holds a timeline answer");
    int64_t* h_out = reinterpret_cast<int64_t*>(f.h_hits);
    HIP_TRY(launch_timeline(a, grid, f.d_part, st), WAX_HIP_ERR_INTERNAL, "timeline launch");
    HIP_TRY(hipMemcpyAsync(h_out, d_out, (size_t)out_words * sizeof(int64_t), hipMemcpyDeviceToHost, st), WAX_HIP_ERR_INTERNAL, "timeline download");
    HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "timeline failed on device");
    const uint32_t n = *reinterpret_cast<const uint32_t*>(h_out + 2 * (size_t)want);
    if (n > (uint32_t)want) return fail(WAX_HIP_ERR_INTERNAL, "timeline: the device returned more rows than asked for");
    std::memcpy(out_ids, h_out, (size_t)n * sizeof(uint64_t));
    if (out_timestamps) std::memcpy(out_timestamps, h_out + want, (size_t)n * sizeof(int64_t));
    *out_count = n;
    return WAX_HIP_OK;
}

int wax_hip_timeline_device(wax_hip_engine* e, int32_t limit, int newest_first, const wax_hip_row_predicate* pred, uint64_t* d_out_ids,
                            uint32_t* d_out_count, void* stream) {
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (!d_out_count || (!d_out_ids && limit > 0)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null device buffer");
    SHARDED_UNSUPPORTED(e, "wax_hip_timeline_device");
    { const int lrc = timeline_refuse_limit(limit); if (lrc != WAX_HIP_OK) return lrc; }
    DeviceGuard g(e->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (limit <= 0) {
        HIP_TRY(hipMemsetAsync(d_out_count, 0, sizeof(uint32_t), st), WAX_HIP_ERR_INTERNAL, "timeline count");
        return WAX_HIP_OK;
    }
    ReadGuard rd(e);
    { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return frc; }
    wax_hip_engine::TimelineRing& t = e->tl_ring[e->tl_next.fetch_add(1) % kShardRing];
    // One user of an entry at a time; its previous use must have finished on ITS stream before the partials are reused.
    std::unique_lock<std::mutex> tg(t.mu);
    if (t.busy) {
        const hipError_t werr = hipEventSynchronize(t.done);
        t.busy = false;
        HIP_TRY(werr, WAX_HIP_ERR_INTERNAL, "timeline scratch wait");
    }
    if (!t.done) HIP_TRY(hipEventCreateWithFlags(&t.done, hipEventDisableTiming), WAX_HIP_ERR_ALLOC, "Failed to allocate timeline events");
    if (!t.cols) HIP_TRY(hipEventCreateWithFlags(&t.cols, hipEventDisableTiming), WAX_HIP_ERR_ALLOC, "Failed to allocate timeline events");
    TimelineArgs a;
    timeline_args(&a, pred, limit, newest_first);
    if (e->count != 0 && e->cols.has_attributes()) {
        // The columns are brought up to date on a workspace stream, as the blocking predicate search does it, and the caller's stream
        // waits for that by an event: an upload on the caller's stream would let a concurrent predicate search (which takes the
        // columns as current once ensure_attrs has returned) read rows another stream is still writing.
        FilterLease lease(e);
        if (lease.rc != WAX_HIP_OK) return lease.rc;
        { const int arc = ensure_attrs(e, lease.work().stream, &a.ts, &a.flags); if (arc != WAX_HIP_OK) return arc; }
        HIP_TRY(hipEventRecord(t.cols, lease.work().stream), WAX_HIP_ERR_INTERNAL, "timeline column event");
        HIP_TRY(hipStreamWaitEvent(st, t.cols, 0), WAX_HIP_ERR_INTERNAL, "timeline column wait");
    }
    a.ids = e->d_ids; a.n_rows = e->count;
    a.out_ids = d_out_ids; a.out_ts = nullptr; a.out_count = d_out_count;
    const uint32_t grid = timeline_grid(e->count, limit);
    { const int grc = grow_dev(&t.d, &t.words, timeline_scratch_words(grid, limit), sizeof(int64_t), "Failed to allocate timeline partials"); if (grc != WAX_HIP_OK) return grc; }
    const hipError_t lerr = launch_timeline(a, grid, t.d, st);
    // whatever was enqueued must drain before the entry is reused or a writer moves the rows
    if (hipEventRecord(t.done, st) == hipSuccess) t.busy = true;
    else (void)hipStreamSynchronize(st);
    HIP_TRY(lerr, WAX_HIP_ERR_INTERNAL, "timeline launch");
    return WAX_HIP_OK;
}

int wax_hip_timeline_probe(const int64_t* timestamps, const uint32_t* flags, const uint64_t* frame_ids, uint64_t n_rows, int32_t limit,
                           int newest_first, const wax_hip_row_predicate* pred, uint32_t grid, uint64_t* out_ids, int64_t* out_timestamps,
                           uint32_t* out_count) {
    if (!out_ids || !out_count || (!frame_ids && n_rows)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    { const int lrc = timeline_refuse_limit(limit); if (lrc != WAX_HIP_OK) return lrc; }
    if (grid > TIMELINE_MAX_GRID) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "timeline_probe: at most 1024 workgroups");
    if (n_rows > 0xffffffffull) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "timeline_probe: at most 2^32 - 1 rows");
    *out_count = 0;
    if (limit <= 0) return WAX_HIP_OK;
    if (grid == 0) grid = timeline_grid(n_rows, limit);
    const uint64_t scratch = timeline_scratch_words(grid, limit), out_words = 2ull * (uint64_t)limit + 1ull;
    const uint64_t ts_words = timestamps ? n_rows : 0, fl_words = flags ? (n_rows + 1ull) / 2ull : 0;
    int64_t* d = nullptr;
    HIP_TRY(hipMalloc(&d, (size_t)(scratch + out_words + n_rows + ts_words + fl_words + 1ull) * sizeof(int64_t)), WAX_HIP_ERR_INTERNAL, "timeline_probe allocation");
    int64_t* d_out = d + scratch;
    uint64_t* d_ids = reinterpret_cast<uint64_t*>(d_out + out_words);
    int64_t* d_ts = reinterpret_cast<int64_t*>(d_ids + n_rows);
    uint32_t* d_fl = reinterpret_cast<uint32_t*>(d_ts + ts_words);
    TimelineArgs a;
    timeline_args(&a, pred, limit, newest_first);
    a.ts = timestamps ? d_ts : nullptr; a.flags = flags ? d_fl : nullptr; a.ids = d_ids; a.n_rows = n_rows;
    a.out_ids = reinterpret_cast<uint64_t*>(d_out); a.out_ts = d_out + limit; a.out_count = reinterpret_cast<uint32_t*>(d_out + 2 * (size_t)limit);
    std::vector<int64_t> h_out((size_t)out_words);
    hipError_t err = hipSuccess;
    if (n_rows) err = hipMemcpy(d_ids, frame_ids, (size_t)n_rows * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (err == hipSuccess && timestamps && n_rows) err = hipMemcpy(d_ts, timestamps, (size_t)n_rows * sizeof(int64_t), hipMemcpyHostToDevice);
    if (err == hipSuccess && flags && n_rows) err = hipMemcpy(d_fl, flags, (size_t)n_rows * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = launch_timeline(a, grid, d, nullptr);
    if (err == hipSuccess) err = hipMemcpy(h_out.data(), d_out, (size_t)out_words * sizeof(int64_t), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIP_TRY(err, WAX_HIP_ERR_INTERNAL, "timeline_probe");
    const uint32_t n = *reinterpret_cast<const uint32_t*>(h_out.data() + 2 * (size_t)limit);
    if (n > (uint32_t)limit) return fail(WAX_HIP_ERR_INTERNAL, "timeline_probe: the device returned more rows than asked for");
    std::memcpy(out_ids, h_out.data(), (size_t)limit * sizeof(uint64_t));   // the padding too
    if (out_timestamps) std::memcpy(out_timestamps, h_out.data() + limit, (size_t)limit * sizeof(int64_t));
    *out_count = n;
    return WAX_HIP_OK;
}
