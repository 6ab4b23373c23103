// api_predicate.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: per-row attributes (set / get) and their device columns (DESIGN 2, 4.5); the predicate search that reads them is in filter_host.inc

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
    sync_timeline_work(e);
    uint64_t applied = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const int64_t r = e->idmap.find(frame_ids[i]);
        if (r < 0) continue;                                   // a frame without a vector has no row to describe
        ++applied;
        if (!timestamps && !flags) continue;
        e->cols.set_attributes((uint64_t)r, e->count, timestamps ? timestamps + i : nullptr, flags ? flags + i : nullptr);
    }
    if (out_applied) *out_applied = applied;
    return WAX_HIP_OK;
}

int wax_hip_get_attributes(wax_hip_engine* e, const uint64_t* frame_ids, uint64_t n, int64_t* out_timestamps, uint32_t* out_flags,
                           uint8_t* out_found) {
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (n == 0) return WAX_HIP_OK;
    if (!frame_ids) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "getAttributes: null input");
    if (e->sh) return sh_get_attributes(e, frame_ids, n, out_timestamps, out_flags, out_found);
    ReadGuard rd(e);
    for (uint64_t i = 0; i < n; ++i) {
        const int64_t r = e->idmap.find(frame_ids[i]);
        if (out_timestamps) out_timestamps[i] = r >= 0 ? e->cols.ts().at((uint64_t)r) : 0;
        if (out_flags) out_flags[i] = r >= 0 ? e->cols.flags().at((uint64_t)r) : 0u;
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
    UploadMark& mark = e->cols.attr_mark();
    const uint64_t na = e->cols.attr_rows(), count = e->count;
    if (na == 0) return WAX_HIP_OK;
    if (e->attr_cap < count) {
        // growth: columns of the store's capacity; the rows that were up to date are kept (a device copy), the rest is uploaded below
        const uint64_t cap = e->capacity > count ? e->capacity : count;
        const uint64_t keep = mark.from(e->attr_cap);
        int64_t* nt = nullptr;
        uint32_t* nf = nullptr;
        HIP_TRY(hipMalloc(&nt, (size_t)cap * sizeof(int64_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate the timestamp column");
        hipError_t err = hipMalloc(&nf, (size_t)cap * sizeof(uint32_t));
        if (err == hipSuccess && keep > 0) err = hipMemcpyAsync(nt, e->d_attr_ts, (size_t)keep * sizeof(int64_t), hipMemcpyDeviceToDevice, st);
        if (err == hipSuccess && keep > 0) err = hipMemcpyAsync(nf, e->d_attr_flags, (size_t)keep * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        if (err != hipSuccess) { (void)hipFree(nt); (void)hipFree(nf); return fail(WAX_HIP_ERR_ALLOC, std::string("Failed to allocate the flag column: ") + hipGetErrorString(err)); }
        (void)hipFree(e->d_attr_ts); (void)hipFree(e->d_attr_flags);
        e->d_attr_ts = nt; e->d_attr_flags = nf; e->attr_cap = cap;
        mark.note(keep);                                       // the new columns hold nothing from there on
    }
    const uint64_t from = mark.from(count);
    if (from < count) {
        const uint64_t host_end = std::min(na, count);         // rows behind the host columns are (0, 0)
        if (from < host_end) {
            // pageable sources: the runtime stages them before returning
            HIP_TRY(hipMemcpyAsync(e->d_attr_ts + from, e->cols.ts().data() + from, (size_t)(host_end - from) * sizeof(int64_t), hipMemcpyHostToDevice, st),
                    WAX_HIP_ERR_INTERNAL, "timestamp upload");
            HIP_TRY(hipMemcpyAsync(e->d_attr_flags + from, e->cols.flags().data() + from, (size_t)(host_end - from) * sizeof(uint32_t), hipMemcpyHostToDevice, st),
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
    mark.settle(count);
    *d_ts = e->d_attr_ts; *d_flags = e->d_attr_flags;
    return WAX_HIP_OK;
}
