// store_internal.inc — part of engine.hip's translation unit (included there; not compiled alone).
// the store behind the C ABI: clampTopK, the scratch-slot pool, the general-selection workspace, staged appends, growth (MetalVectorEngine.swift:84-117, 330-357, 842-890)

int clamp_topk(int64_t top_k) {  // MetalVectorEngine.swift:842-846
    if (top_k < 1) return 1;
    if (top_k > WAX_HIP_MAX_RESULTS) return WAX_HIP_MAX_RESULTS;
    return (int)top_k;
}

std::string dim_mismatch_msg(uint32_t expected, uint64_t got) {  // MetalVectorEngine.swift:832
    return "vector dimension mismatch: expected " + std::to_string(expected) + ", got " + std::to_string(got);
}

int alloc_slot(wax_hip_engine* e, Slot** out) {
    Slot* s = new Slot();
    auto bail = [&](int code, const char* what, hipError_t err) {
        std::string msg = std::string("Failed to allocate ") + what + ": " + hipGetErrorString(err);
        if (s->ev0) (void)hipEventDestroy(s->ev0);
        if (s->ev1) (void)hipEventDestroy(s->ev1);
        if (s->ev_done) (void)hipEventDestroy(s->ev_done);
        (void)hipFree(s->d_query); (void)hipHostFree(s->h_query); (void)hipFree(s->d_partials);
        (void)hipFree(s->d_hits); (void)hipHostFree(s->h_hits); (void)hipHostFree(s->h_done);
        delete s;
        return fail(code, msg);
    };
    hipError_t err;
    // kernel-timing events: device-scope release (no system-scope cache flush folded into the interval or into the
    // gap before the next scan); ev_done is what the host waits on for results in pinned memory: default (system) scope
    if ((err = hipEventCreateWithFlags(&s->ev0, hipEventReleaseToDevice)) != hipSuccess) return bail(WAX_HIP_ERR_ALLOC, "event", err);
    if ((err = hipEventCreateWithFlags(&s->ev1, hipEventReleaseToDevice)) != hipSuccess) return bail(WAX_HIP_ERR_ALLOC, "event", err);
    if ((err = hipEventCreateWithFlags(&s->ev_done, hipEventDisableTiming)) != hipSuccess) return bail(WAX_HIP_ERR_ALLOC, "event", err);
    const size_t qbytes = (size_t)e->dims * sizeof(float);
    if ((err = hipMalloc(&s->d_query, qbytes)) != hipSuccess) return bail(WAX_HIP_ERR_ALLOC, "transient query buffer", err);
    // (device-mapped, as hipHostMallocDefault is: mirror_group_queries_kernel reads a parked query straight from h_query)
    if ((err = hipHostMalloc(&s->h_query, qbytes, hipHostMallocDefault | hipHostMallocMapped)) != hipSuccess) return bail(WAX_HIP_ERR_ALLOC, "pinned query buffer", err);
    if ((err = hipMalloc(&s->d_partials, kPartialsBytes)) != hipSuccess) return bail(WAX_HIP_ERR_ALLOC, "top-k stage buffer", err);
    if ((err = hipMemset(partials_ticket(s->d_partials), 0, 128)) != hipSuccess) return bail(WAX_HIP_ERR_ALLOC, "top-k stage buffer", err);
    // hipMemset on device memory may return before the fill has run, and the slot's scans run on non-blocking streams the
    // null stream does not order against: wait once, here, so the first fused scan can only ever see an armed (zero) ticket
    if ((err = hipStreamSynchronize(nullptr)) != hipSuccess) return bail(WAX_HIP_ERR_ALLOC, "top-k stage buffer", err);
    if ((err = hipMalloc(&s->d_hits, (size_t)WAX_HIP_MAX_RESULTS * sizeof(wax_hip_hit))) != hipSuccess) return bail(WAX_HIP_ERR_ALLOC, "top-k results buffer", err);
    // The completion-word protocol ("done_flag") needs the kernel's writes — hits, then the word — visible to the host IN ORDER while
    // the kernel is still running: coherent (fine-grained) host memory, asked for explicitly (the default is coherent on this stack
    // today, but HIP_HOST_COHERENT=0 or another platform changes that silently). Where a coherent allocation is refused the slot falls
    // back to default pinned memory and never takes the completion-word path (collect waits on the event behind the kernel).
    s->coherent = true;
    if ((err = hipHostMalloc(&s->h_hits, (size_t)WAX_HIP_MAX_RESULTS * sizeof(wax_hip_hit), hipHostMallocCoherent)) != hipSuccess) {
        (void)hipGetLastError();
        s->coherent = false;
        if ((err = hipHostMalloc(&s->h_hits, (size_t)WAX_HIP_MAX_RESULTS * sizeof(wax_hip_hit), hipHostMallocDefault)) != hipSuccess) return bail(WAX_HIP_ERR_ALLOC, "pinned results buffer", err);
    }
    if ((err = hipHostMalloc(&s->h_done, 64, s->coherent ? hipHostMallocCoherent : hipHostMallocDefault)) != hipSuccess) {
        (void)hipGetLastError();
        s->coherent = false;
        if ((err = hipHostMalloc(&s->h_done, 64, hipHostMallocDefault)) != hipSuccess) return bail(WAX_HIP_ERR_ALLOC, "pinned completion word", err);
    }
    *s->h_done = 0;
    *out = s;
    return WAX_HIP_OK;
}

void free_slot(Slot* s) {
    if (!s) return;
    (void)hipFree(s->d_query); (void)hipHostFree(s->h_query); (void)hipFree(s->d_partials);
    (void)hipFree(s->d_hits); (void)hipHostFree(s->h_hits); (void)hipHostFree(s->h_done); (void)hipFree(s->d_dist);
    if (s->sw_ready) free_select_work(&s->sw);
    (void)hipEventDestroy(s->ev0); (void)hipEventDestroy(s->ev1); (void)hipEventDestroy(s->ev_done);
    delete s;
}

// acquireTransientBuffers (MetalVectorEngine.swift:84-113): reuse a pooled slot or create one.
constexpr int kSlotBusy = 1;  // internal: try_only and every slot is in use

// `holder`: the calling thread already owns tickets (= slots), so it never WAITS for one (work_pool.h, PoolMode::grow). Like the
// reference's transient buffer pool (MetalVectorEngine.swift:84-117: an empty pool allocates) it gets a freshly allocated slot beyond
// "slots" (counted in transient_allocations; the slot stays pooled afterwards), up to kHardSlotCap. Returned by e->slots.release(s)
// (releaseTransientBuffers, :115-117).
int take_slot(wax_hip_engine* e, Slot** out, bool try_only = false, bool holder = false) {
    int rc = WAX_HIP_OK;
    switch (e->slots.acquire(try_only ? PoolMode::tries : holder ? PoolMode::grow : PoolMode::wait, out, &rc, [e](int index, Slot** made) {
        const int mrc = alloc_slot(e, made);
        if (mrc == WAX_HIP_OK) (*made)->index = index;
        return mrc;
    })) {
    case PoolGot::reused: e->st_reuse++; break;   // idle slot: safe to re-home
    case PoolGot::fresh: e->st_alloc++; break;
    case PoolGot::busy: return kSlotBusy;
    case PoolGot::exhausted: return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "too many outstanding search tickets (collect some first)");
    case PoolGot::failed: return rc;
    }
    (*out)->stream = e->streams[(*out)->index % e->n_streams];
    return WAX_HIP_OK;
}

int ensure_general(wax_hip_engine* e, Slot* s) {
    if (s->dist_cap < e->capacity) {
        (void)hipStreamSynchronize(s->stream);
        (void)hipFree(s->d_dist);
        s->d_dist = nullptr; s->dist_cap = 0;
        HIP_TRY(hipMalloc(&s->d_dist, (size_t)e->capacity * sizeof(float)), WAX_HIP_ERR_ALLOC,
                "Failed to allocate transient distances buffer");
        s->dist_cap = e->capacity;
    }
    if (!s->sw_ready) {
        HIP_TRY(alloc_select_work(&s->sw), WAX_HIP_ERR_ALLOC, "Failed to allocate the selection workspace");
        s->sw_ready = true;
    }
    return WAX_HIP_OK;
}

// ||q|| in f64, four independent partial sums (a single chain is add-latency-bound: 0.16 us per 384-d query,
// 160 us for a 1024-query batch). Every path (single query, batch re-score) takes its norm from here.
float query_norm(const float* q, uint32_t dims) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    uint32_t j = 0;
    for (; j + 4 <= dims; j += 4) {
        s0 += (double)q[j] * (double)q[j];
        s1 += (double)q[j + 1] * (double)q[j + 1];
        s2 += (double)q[j + 2] * (double)q[j + 2];
        s3 += (double)q[j + 3] * (double)q[j + 3];
    }
    for (; j < dims; ++j) s0 += (double)q[j] * (double)q[j];
    return (float)std::sqrt((s0 + s1) + (s2 + s3));
}

// Upload the staged appends. Callers hold the engine lock (shared or exclusive); readers may race each other here,
// never a writer (staging is only filled under the exclusive lock). Rows >= count - pend_rows are beyond the n_rows of
// every scan already in flight, so writing them concurrently with those scans is safe.
int flush_pending(wax_hip_engine* e) {
    if (e->pend_rows.load(std::memory_order_acquire) == 0) return WAX_HIP_OK;
    std::unique_lock<std::mutex> g(e->pend_mu);
    const uint64_t n = e->pend_rows.load(std::memory_order_relaxed);
    if (n == 0) return WAX_HIP_OK;
    const uint64_t first = e->count - n;
    HIP_TRY(hipMemcpy(e->d_store + first * e->dims, e->h_pend, (size_t)n * e->dims * sizeof(float), hipMemcpyHostToDevice),
            WAX_HIP_ERR_INTERNAL, "vector upload");
    HIP_TRY(hipMemcpy(e->d_ids + first, e->ids.data() + first, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice),
            WAX_HIP_ERR_INTERNAL, "frame id upload");
    e->pend_rows.store(0, std::memory_order_release);
    return WAX_HIP_OK;
}

// resizeBuffersIfNeeded (MetalVectorEngine.swift:873-890): new slab + copy of the live rows.
int resize_store(wax_hip_engine* e, uint64_t new_cap) {
    if (new_cap <= e->capacity) return WAX_HIP_OK;
    { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return frc; }   // the copy below reads device rows
    float* ns = nullptr;
    uint64_t* ni = nullptr;
    const size_t row_bytes = (size_t)e->dims * sizeof(float);
    hipError_t err = hipMalloc(&ns, (size_t)new_cap * row_bytes);
    if (err != hipSuccess) return fail(WAX_HIP_ERR_ALLOC, std::string("Failed to resize vectors buffer: ") + hipGetErrorString(err));
    err = hipMalloc(&ni, (size_t)new_cap * sizeof(uint64_t));
    if (err != hipSuccess) { (void)hipFree(ns); return fail(WAX_HIP_ERR_ALLOC, std::string("Failed to resize frame id buffer: ") + hipGetErrorString(err)); }
    if (e->count > 0) {
        err = hipMemcpy(ns, e->d_store, (size_t)e->count * row_bytes, hipMemcpyDeviceToDevice);
        if (err == hipSuccess) err = hipMemcpy(ni, e->d_ids, (size_t)e->count * sizeof(uint64_t), hipMemcpyDeviceToDevice);
        if (err != hipSuccess) { (void)hipFree(ns); (void)hipFree(ni); return fail(WAX_HIP_ERR_INTERNAL, std::string("store copy failed: ") + hipGetErrorString(err)); }
    }
    (void)hipFree(e->d_store); (void)hipFree(e->d_ids);
    e->d_store = ns; e->d_ids = ni; e->capacity = new_cap;
    return WAX_HIP_OK;
}

// reserveIfNeeded (MetalVectorEngine.swift:857-871)
int reserve_rows(wax_hip_engine* e, uint64_t required) {
    if (required > 0xffffffffull)
        return fail(WAX_HIP_ERR_CAPACITY, "capacity exceeded: limit 4294967295, requested " + std::to_string(required));
    if (required <= e->capacity) return WAX_HIP_OK;
    uint64_t next = e->capacity == 0 ? WAX_HIP_INITIAL_RESERVE : e->capacity;
    while (required > next) {
        uint64_t doubled = next * 2;
        next = doubled > 0xffffffffull ? 0xffffffffull : doubled;
        if (next == 0xffffffffull) break;
    }
    return resize_store(e, next);
}

