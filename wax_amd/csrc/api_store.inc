// api_store.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: availability, create / destroy, accessors, reserve / add / add_batch / add_batch_device / apply_put_embeddings / remove / remove_batch

// ===========================================================================
// C ABI
extern "C" {

int wax_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int wax_hip_available(void) {
    const int n = wax_hip_device_count();
    for (int d = 0; d < n; ++d)
        if (device_is_gfx950(d)) return 1;
    return 0;
}

uint32_t wax_hip_abi_version(void) { return WAX_HIP_ABI_VERSION; }

const char* wax_hip_last_error(void) { return g_last_error.c_str(); }

int wax_hip_engine_create(uint8_t metric, uint32_t dims, int device_id, wax_hip_engine** out) {
    if (!out) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    if (dims == 0) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "dimensions must be > 0");  // :154-156
    if (dims > WAX_HIP_MAX_DIMENSIONS)                                                     // :157-162
        return fail(WAX_HIP_ERR_CAPACITY, "capacity exceeded: limit " + std::to_string(WAX_HIP_MAX_DIMENSIONS) +
                                              ", requested " + std::to_string(dims));
    if (metric > WAX_HIP_METRIC_L2) return fail(WAX_HIP_ERR_METRIC_UNSUPPORTED, "unsupported metric " + std::to_string((int)metric));
    const int n = wax_hip_device_count();
    if (n <= 0) return fail(WAX_HIP_ERR_NO_DEVICE, "HIP device not available");          // :167-169
    int dev = device_id;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    }
    if (dev >= n) return fail(WAX_HIP_ERR_NO_DEVICE, "HIP device " + std::to_string(dev) + " not available");
    if (!device_is_gfx950(dev)) return fail(WAX_HIP_ERR_NO_DEVICE, "HIP device " + std::to_string(dev) + " is not gfx950 (MI355X)");

    DeviceGuard g(dev);
    wax_hip_engine* e = new wax_hip_engine();
    e->device = dev;
    e->metric = metric;
    e->dims = dims;
    if (const char* v = std::getenv("WAX_HIP_BATCH_REGA")) {  // default of the "batch_rega" tunable (A/B runs of the whole test suite)
        const std::string keep = g_last_error;                // a value the key's row (tuning.inc) refuses is ignored silently
        // (e->sh is still null here, also for a shard of a handle: the call cannot be handed over to the sharded path)
        if (wax_hip_set_tuning(e, "batch_rega", std::strtol(v, nullptr, 10)) != WAX_HIP_OK) g_last_error = keep;
    }
    int rc = resize_store(e, WAX_HIP_INITIAL_RESERVE);  // :225-229
    if (rc == WAX_HIP_OK) {
        hipError_t err = hipMalloc(&e->d_sink, MAX_GRID_BLOCKS * sizeof(float));
        if (err != hipSuccess) rc = fail(WAX_HIP_ERR_ALLOC, std::string("Failed to allocate sink: ") + hipGetErrorString(err));
    }
    if (rc == WAX_HIP_OK) {
        // Timing stays ENABLED on purpose: the runtime gives a timing event its own completion signal, so a stream
        // waiting on it resumes when the scan ends. A hipEventDisableTiming event was observed to resolve only with
        // the next command of the recording stream (the merge kernel): +13 us of idle HBM per query.
        hipError_t err = hipEventCreateWithFlags(&e->scan_done, hipEventReleaseToDevice);
        if (err != hipSuccess) rc = fail(WAX_HIP_ERR_ALLOC, std::string("Failed to create event: ") + hipGetErrorString(err));
    }
    for (int i = 0; i < kMaxStreams && rc == WAX_HIP_OK; ++i) {
        hipError_t err = hipStreamCreateWithFlags(&e->streams[i], hipStreamNonBlocking);
        if (err != hipSuccess) rc = fail(WAX_HIP_ERR_ALLOC, std::string("Failed to create stream: ") + hipGetErrorString(err));
    }
    if (rc == WAX_HIP_OK) {
        Slot* s = nullptr;
        rc = alloc_slot(e, &s);  // one pooled slot up front, like transientBufferPool's seed entry (:266-273)
        if (rc == WAX_HIP_OK) {
            s->index = 0;
            s->stream = e->streams[0];
            e->slots.seed(s);
        }
    }
    if (rc != WAX_HIP_OK) {
        wax_hip_engine_destroy(e);
        return rc;
    }
    *out = e;
    return WAX_HIP_OK;
}

void wax_hip_engine_destroy(wax_hip_engine* e) {
    if (!e) return;
    if (e->sh) { sh_destroy(e); delete e; return; }
    DeviceGuard g(e->device);
    (void)hipDeviceSynchronize();
    e->slots.drain(free_slot);
    for (int i = 0; i < kMaxStreams; ++i)
        if (e->streams[i]) (void)hipStreamDestroy(e->streams[i]);
    if (e->scan_done) (void)hipEventDestroy(e->scan_done);
    for (hipEvent_t ev : e->tev) if (ev) (void)hipEventDestroy(ev);
    if (e->h_pend) (void)hipHostFree(e->h_pend);
    for (int i = 0; i < kShardRing; ++i) {
        (void)hipFree(e->ring_d_query[i]);
        (void)hipHostFree(e->ring_h_query[i]);
        (void)hipFree(e->ring_d_partials[i]);
        if (e->ring_ev0[i]) (void)hipEventDestroy(e->ring_ev0[i]);
        if (e->ring_ev1[i]) (void)hipEventDestroy(e->ring_ev1[i]);
        if (e->ring_done[i]) (void)hipEventDestroy(e->ring_done[i]);
    }
    for (auto& t : e->tl_ring) {
        (void)hipFree(t.d);
        if (t.done) (void)hipEventDestroy(t.done);
        if (t.cols) (void)hipEventDestroy(t.cols);
    }
    {
        BatchMirror& b = e->batch;
        (void)hipFree(b.d_cb); (void)hipFree(b.d_vn2); (void)hipFree(b.d_maxnorm); (void)hipFree(b.d_dirty);
        if (b.ev_ready) (void)hipEventDestroy(b.ev_ready);
        (void)hipFree(b.d_c8); (void)hipFree(b.d_c8_meta); (void)hipFree(b.d_c8_max);
        if (b.ev8_ready) (void)hipEventDestroy(b.ev8_ready);
        e->bctxs.drain(free_bctx);
        e->filter_works.drain(free_filter_work);
        (void)hipFree(e->idhash.d_table);
        (void)hipFree(e->d_attr_ts); (void)hipFree(e->d_attr_flags);
        (void)hipFree(e->d_grp_slot); (void)hipFree(e->d_grp_root);
        (void)hipFree(e->d_term_off); (void)hipFree(e->d_term_val);
        for (PredEntry& p : e->pred_entries) {
            (void)hipFree(p.d_bitmap); (void)hipFree(p.d_counts); (void)hipHostFree(p.h_counts);
            if (p.built_ev) (void)hipEventDestroy(p.built_ev);
        }
    }
    (void)hipFree(e->d_store);
    (void)hipFree(e->d_ids);
    (void)hipFree(e->d_sink);
    (void)hipFree(e->d_bounce);
    delete e;
}

uint32_t wax_hip_dimensions(const wax_hip_engine* e) { return e ? e->dims : 0; }
uint64_t wax_hip_count(const wax_hip_engine* e) { return e ? (e->sh ? sh_total_count(e) : e->count) : 0; }
uint8_t wax_hip_metric_of(const wax_hip_engine* e) { return e ? e->metric : 0; }
int wax_hip_device_of(const wax_hip_engine* e) { return e ? e->device : -1; }

// ---- mutation -------------------------------------------------------------

int wax_hip_reserve(wax_hip_engine* e, uint64_t rows) {
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (e->sh) return sh_reserve(e, rows);
    REFUSE_IF_HOLDING(e);
    DeviceGuard g(e->device);
    WriteGuard w(e->lock);
    sync_shard_work(e);
    int rc = reserve_rows(e, rows);
    if (rc == WAX_HIP_OK) e->idmap.reserve(rows);
    return rc;
}

int wax_hip_add_batch(wax_hip_engine* e, const uint64_t* frame_ids, const float* rows, uint64_t n, uint32_t dims) {
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (e->sh) return sh_add_batch(e, frame_ids, rows, n, dims);
    if (n == 0) return WAX_HIP_OK;  // :360
    if (!frame_ids || !rows) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "addBatch: null input");
    if (dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));  // :367-370
    REFUSE_IF_HOLDING(e);
    DeviceGuard g(e->device);
    WriteGuard w(e->lock);
    sync_shard_work(e);
    e->derived.appended();
    const size_t row_bytes = (size_t)e->dims * sizeof(float);
    if (n == 1) {
        // add(frameId:vector:) (:330-357): no device call at all on the common paths — the row goes to the staging
        // area and reaches HBM with the next reader (one copy for all rows added since)
        const int64_t existing = e->idmap.find(frame_ids[0]);
        const uint64_t pend = e->pend_rows.load(std::memory_order_relaxed);
        if (existing >= 0) {
            if ((uint64_t)existing >= e->count - pend) {     // still staged: overwrite in place
                std::memcpy(e->h_pend + ((uint64_t)existing - (e->count - pend)) * e->dims, rows, row_bytes);
            } else {
                HIP_TRY(hipMemcpy(e->d_store + (uint64_t)existing * e->dims, rows, row_bytes, hipMemcpyHostToDevice),
                        WAX_HIP_ERR_INTERNAL, "vector upload");
            }
            e->derived.overwritten((uint64_t)existing);
            return WAX_HIP_OK;
        }
        int rc1 = reserve_rows(e, e->count + 1);             // :341 (flushes before it reallocates)
        if (rc1 != WAX_HIP_OK) return rc1;
        if (!e->h_pend) {
            uint64_t cap = (8ull << 20) / row_bytes;
            if (cap < 1) cap = 1;
            if (cap > 65536) cap = 65536;
            HIP_TRY(hipHostMalloc(&e->h_pend, (size_t)cap * row_bytes, hipHostMallocDefault), WAX_HIP_ERR_ALLOC,
                    "Failed to allocate append staging buffer");
            e->pend_cap = cap;
        }
        if (e->pend_rows.load(std::memory_order_relaxed) == e->pend_cap) {
            rc1 = flush_pending(e);
            if (rc1 != WAX_HIP_OK) return rc1;
        }
        const uint64_t slot = e->pend_rows.load(std::memory_order_relaxed);
        std::memcpy(e->h_pend + slot * e->dims, rows, row_bytes);
        e->idmap.put(frame_ids[0], (uint32_t)e->count);
        e->ids.push_back(frame_ids[0]);
        e->count += 1;
        e->pend_rows.store(slot + 1, std::memory_order_release);
        return WAX_HIP_OK;
    }
    int rc = flush_pending(e);               // batch rows go straight to HBM; keep the staged ones in front of them
    if (rc != WAX_HIP_OK) return rc;
    rc = reserve_rows(e, e->count + n);      // :379-380 (upper bound: every id new)
    if (rc != WAX_HIP_OK) return rc;
    // Sequential upsert semantics of :384-398; consecutive appends are flushed as one H2D copy.
    uint64_t run_start = 0, run_len = 0;  // pending append run: input rows [run_start, run_start+run_len)
    auto flush = [&]() -> int {
        if (run_len == 0) return WAX_HIP_OK;
        const uint64_t first_row = e->count - run_len;
        HIP_TRY(hipMemcpy(e->d_store + first_row * e->dims, rows + run_start * e->dims, (size_t)run_len * row_bytes,
                          hipMemcpyHostToDevice), WAX_HIP_ERR_INTERNAL, "vector upload");
        HIP_TRY(hipMemcpy(e->d_ids + first_row, e->ids.data() + first_row, (size_t)run_len * sizeof(uint64_t),
                          hipMemcpyHostToDevice), WAX_HIP_ERR_INTERNAL, "frame id upload");
        run_len = 0;
        return WAX_HIP_OK;
    };
    for (uint64_t i = 0; i < n; ++i) {
        const int64_t existing = e->idmap.find(frame_ids[i]);
        if (existing >= 0) {
            if ((rc = flush()) != WAX_HIP_OK) return rc;
            HIP_TRY(hipMemcpy(e->d_store + (uint64_t)existing * e->dims, rows + i * e->dims, row_bytes,
                              hipMemcpyHostToDevice), WAX_HIP_ERR_INTERNAL, "vector upload");
            e->derived.overwritten((uint64_t)existing);
        } else {
            if (run_len == 0) run_start = i;
            e->idmap.put(frame_ids[i], (uint32_t)e->count);
            e->ids.push_back(frame_ids[i]);
            e->count += 1;
            run_len += 1;
        }
    }
    return flush();
}

int wax_hip_add(wax_hip_engine* e, uint64_t frame_id, const float* vector, uint32_t dims) {
    return wax_hip_add_batch(e, &frame_id, vector, 1, dims);  // :330-357 is the n == 1 case of :359-402
}

int wax_hip_add_batch_device(wax_hip_engine* e, const uint64_t* frame_ids, const float* d_rows, uint64_t n, uint32_t dims) {
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (e->sh) return sh_add_batch_device(e, frame_ids, d_rows, n, dims);
    if (n == 0) return WAX_HIP_OK;
    if (!frame_ids || !d_rows) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "addBatch: null input");
    if (dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));
    REFUSE_IF_HOLDING(e);
    DeviceGuard g(e->device);
    WriteGuard w(e->lock);
    sync_shard_work(e);
    e->derived.appended();
    { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return frc; }
    for (uint64_t i = 0; i < n; ++i)
        if (e->idmap.find(frame_ids[i]) >= 0)
            return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "add_batch_device: frame id " + std::to_string(frame_ids[i]) + " already present (append-only path)");
    int rc = reserve_rows(e, e->count + n);
    if (rc != WAX_HIP_OK) return rc;
    const uint64_t first_row = e->count;
    // Failure-atomic: duplicates inside the batch are detected on a scratch map, the rows and ids reach HBM next, and the
    // host bookkeeping (ids, id map, count) is committed only after both copies succeeded — a failed copy leaves the
    // engine exactly as it was (the bytes written past `count` are invisible to every reader).
    {
        IdMap seen;
        seen.reserve((size_t)n);
        for (uint64_t i = 0; i < n; ++i) {
            if (seen.find(frame_ids[i]) >= 0)
                return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "add_batch_device: duplicate frame id " + std::to_string(frame_ids[i]) + " inside batch");
            seen.put(frame_ids[i], 0);
        }
    }
    HIP_TRY(hipMemcpy(e->d_store + first_row * e->dims, d_rows, (size_t)n * e->dims * sizeof(float), hipMemcpyDeviceToDevice),
            WAX_HIP_ERR_INTERNAL, "vector copy");
    HIP_TRY(hipMemcpy(e->d_ids + first_row, frame_ids, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice),
            WAX_HIP_ERR_INTERNAL, "frame id upload");
    e->ids.reserve(e->ids.size() + n);
    e->idmap.reserve((size_t)(first_row + n));
    for (uint64_t i = 0; i < n; ++i) {
        e->idmap.put(frame_ids[i], (uint32_t)(first_row + i));
        e->ids.push_back(frame_ids[i]);
    }
    e->count += n;
    return WAX_HIP_OK;
}

int wax_hip_apply_put_embeddings(wax_hip_engine* e, const uint8_t* payloads, uint64_t len, uint64_t* out_applied) {
    if (out_applied) *out_applied = 0;
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (len == 0) return WAX_HIP_OK;
    if (!payloads) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "applyPutEmbeddings: null input");
    constexpr uint64_t kHead = 1 + 8 + 4;  // opcode, frameId, dimension (WALEntryCodec.swift:39-42)
    std::vector<uint64_t> ids;
    std::vector<uint64_t> offs;  // byte offset of each record's f32 payload
    uint64_t pos = 0;
    while (pos < len) {
        if (payloads[pos] != 0x04) {
            char b[64];
            snprintf(b, sizeof b, "unknown opcode 0x%02X at byte %llu", payloads[pos], (unsigned long long)pos);
            return fail(WAX_HIP_ERR_BAD_SEGMENT, payloads[pos] >= 0x01 && payloads[pos] <= 0x03
                                                     ? std::string("not a putEmbedding entry: ") + b : std::string(b));
        }
        if (len - pos < kHead) return fail(WAX_HIP_ERR_BAD_SEGMENT, "truncated putEmbedding header");
        uint64_t id;
        uint32_t dim;
        memcpy(&id, payloads + pos + 1, 8);
        memcpy(&dim, payloads + pos + 9, 4);
        if (dim > WAX_HIP_MAX_DIMENSIONS) return fail(WAX_HIP_ERR_BAD_SEGMENT, "embedding dimension exceeds limit");  // :117-119
        if (dim != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dim));
        const uint64_t bytes = (uint64_t)dim * 4;
        if (len - pos - kHead < bytes) return fail(WAX_HIP_ERR_BAD_SEGMENT, "truncated putEmbedding vector");
        ids.push_back(id);
        offs.push_back(pos + kHead);
        pos += kHead + bytes;
    }
    std::vector<float> rows((size_t)ids.size() * e->dims);
    for (size_t i = 0; i < ids.size(); ++i) memcpy(rows.data() + i * e->dims, payloads + offs[i], (size_t)e->dims * 4);
    const int rc = wax_hip_add_batch(e, ids.data(), rows.data(), ids.size(), e->dims);
    if (rc == WAX_HIP_OK && out_applied) *out_applied = ids.size();
    return rc;
}

int wax_hip_remove(wax_hip_engine* e, uint64_t frame_id) {
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (e->sh) return sh_remove(e, frame_id);
    REFUSE_IF_HOLDING(e);
    DeviceGuard g(e->device);
    WriteGuard w(e->lock);
    sync_shard_work(e);
    if (e->count == 0) return WAX_HIP_OK;                 // :425
    const int64_t idx = e->idmap.find(frame_id);
    if (idx < 0) return WAX_HIP_OK;                       // :426
    { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return frc; }   // the shift below works on device rows
    const uint64_t after = e->count - 1 - (uint64_t)idx;  // :431
    if (after > 0) {
        if (!e->d_bounce)
            HIP_TRY(hipMalloc(&e->d_bounce, kBounceBytes), WAX_HIP_ERR_ALLOC, "Failed to allocate bounce buffer");
        const uint64_t rb = (uint64_t)e->dims * sizeof(float);
        HIP_TRY(device_shift_down(e->d_store, (uint64_t)idx * rb, (uint64_t)(idx + 1) * rb, after * rb, e->d_bounce,
                                  kBounceBytes, nullptr), WAX_HIP_ERR_INTERNAL, "row shift");
        HIP_TRY(device_shift_down(e->d_ids, (uint64_t)idx * 8, (uint64_t)(idx + 1) * 8, after * 8, e->d_bounce,
                                  kBounceBytes, nullptr), WAX_HIP_ERR_INTERNAL, "frame id shift");
        HIP_TRY(hipStreamSynchronize(nullptr), WAX_HIP_ERR_INTERNAL, "row shift sync");
    }
    // the mirror's tail follows the store's; if it cannot, the store has moved all the same: the mirror is converted again at its next
    // use and the host bookkeeping below still runs (returning here would leave ids / count describing the store before the shift)
    const bool followed = mirror_follow_remove(e, (uint64_t)idx) == WAX_HIP_OK;
    if (!followed) (void)hipGetLastError();
    e->derived.removed((uint64_t)idx, followed);
    const bool repeated_ids = e->idmap.size() != e->count;   // only deserialize can put a frame id into several rows
    e->ids.erase(e->ids.begin() + idx);                   // :440
    e->cols.remove_row((uint64_t)idx);                    // the row's entries in the per-row columns go with its id
    e->idmap.erase_row(frame_id, (uint32_t)idx);
    if (repeated_ids) {
        // firstIndex(of:) semantics: the id now means the next row that holds it (the map held the first one, so any other lies behind it)
        const auto next = std::find(e->ids.begin() + idx, e->ids.end(), frame_id);
        if (next != e->ids.end()) e->idmap.put(frame_id, (uint32_t)(next - e->ids.begin()));
    }
    e->count -= 1;                                        // :441
    return WAX_HIP_OK;
}

int wax_hip_remove_batch(wax_hip_engine* e, const uint64_t* frame_ids, uint64_t n, uint64_t* out_removed) {
    if (out_removed) *out_removed = 0;
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (e->sh) return sh_remove_batch(e, frame_ids, n, out_removed);
    if (n == 0) return WAX_HIP_OK;
    if (!frame_ids) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "removeBatch: null input");
    REFUSE_IF_HOLDING(e);
    bool repeated_ids = false;
    {
        DeviceGuard g(e->device);
        WriteGuard w(e->lock);
        sync_shard_work(e);
        if (e->count == 0) return WAX_HIP_OK;                 // :425
        { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return frc; }   // staged rows may be among the ids; the pass works on device rows
        // One id -> one row is what the one-pass map relies on. Only deserialize can put a frame id into several rows, and the id
        // map then holds fewer ids than the store has rows: such a store takes the per-id loop below.
        repeated_ids = e->idmap.size() != e->count;
        if (!repeated_ids) {
            // ---- everything that can fail without touching the store ----
            std::vector<uint32_t> rem;
            rem.reserve((size_t)std::min<uint64_t>(n, e->count));
            for (uint64_t i = 0; i < n; ++i) {
                const int64_t r = e->idmap.find(frame_ids[i]);
                if (r >= 0) rem.push_back((uint32_t)r);        // :426 absent ids are ignored
            }
            std::sort(rem.begin(), rem.end());
            rem.erase(std::unique(rem.begin(), rem.end()), rem.end());   // an id listed twice counts once
            if (rem.empty()) return WAX_HIP_OK;
            const uint64_t m = rem.size();
            BatchMirror& b = e->batch;
            const bool moves = rem[0] + m < e->count;          // false: the removed rows are the store's tail, nothing moves
            uint32_t* d_rem = nullptr;
            bool follow = false;                               // the mirror's rows move with the store's
            uint64_t written = 0;
            if (moves) {
                if (!e->d_bounce)
                    HIP_TRY(hipMalloc(&e->d_bounce, kBounceBytes), WAX_HIP_ERR_ALLOC, "Failed to allocate bounce buffer");
                HIP_TRY(hipMalloc(&d_rem, (size_t)m * sizeof(uint32_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate the removed-row list");
                hipError_t err = hipMemcpy(d_rem, rem.data(), (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice);
                if (err != hipSuccess) { (void)hipFree(d_rem); return fail(WAX_HIP_ERR_INTERNAL, std::string("removed-row list upload: ") + hipGetErrorString(err)); }
                follow = e->derived.bf16.holds(rem[0]);               // (a fill that holds a row has its buffer: mirror_follow_remove)
                if (b.ev_pending) { (void)hipEventSynchronize(b.ev_ready); b.ev_pending = false; }   // a conversion in flight reads the store and writes the mirror
                // ---- the device pass ----
                const int rc = compact_removed_rows(e, rem, d_rem, follow ? e->derived.bf16.rows() : 0, &written);
                (void)hipFree(d_rem);
                if (rc != WAX_HIP_OK) { (void)hipGetLastError(); e->derived.lost(); return rc; }   // (a failed launch or copy: as in remove, the rows behind rem[0] are lost with it)
            } else {
                follow = true;                                 // the mirror's tail is simply cut off with the store's
            }
            // ---- host bookkeeping, committed after the device pass has completed ----
            e->derived.removed(rem.data(), rem.size(), follow);
            for (uint32_t r : rem) e->idmap.erase_only(e->ids[r]);
            e->idmap.renumber_removed(rem, e->count);
            {
                uint64_t wr = rem[0];
                size_t p = 0;
                for (uint64_t r = rem[0]; r < e->count; ++r) {
                    if (p < m && rem[p] == r) { ++p; continue; }
                    e->ids[wr++] = e->ids[r];
                }
                e->ids.resize((size_t)wr);
            }
            e->cols.remove_rows(rem.data(), rem.size());        // the per-row columns: a pass each, over the rows they hold
            e->count -= m;                                     // :441, m times
            e->st_remove_batches += 1;
            e->st_remove_batch_rows += m;
            e->st_remove_batch_bytes += written;
            if (out_removed) *out_removed = m;
            return WAX_HIP_OK;
        }
    }
    // a store with a frame id in several rows: remove(frameId:) per id, exactly the loop this call stands for
    uint64_t removed = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t before = e->count;
        const int rc = wax_hip_remove(e, frame_ids[i]);
        if (rc != WAX_HIP_OK) { if (out_removed) *out_removed = removed; return rc; }
        if (e->count < before) removed += before - e->count;
    }
    if (out_removed) *out_removed = removed;
    return WAX_HIP_OK;
}

