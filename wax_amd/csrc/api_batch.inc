// api_batch.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: search_batch[_hits], the device-resident and ticketed batched entry points


// nq queries -> nq rows of `stride` hits (ascending key, every row KEY_PAD padded to `stride`). Chooses the MFMA path
// when the batch is a genuine GEMM, otherwise pipelines single-query scans over the scratch-slot pool. The row
// count is read under the lock by whichever path runs; the output layout depends on `stride` alone, so a
// concurrent add can never make the library write past the caller's arrays.
static int search_batch_hits_impl(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k,
                                  wax_hip_hit* out_hits, uint32_t stride, uint32_t* out_counts) {
    for (uint32_t q = 0; q < nq; ++q) out_counts[q] = 0;
    for (size_t i = 0; i < (size_t)nq * stride; ++i) out_hits[i] = wax_hip_hit{KEY_PAD, ID_PAD};
    if (stride == 0) return WAX_HIP_OK;
    const uint64_t cnt = e->count;                       // heuristics only; every path re-reads it under the lock
    const uint64_t limit = (uint64_t)clamp_topk(top_k);
    const uint64_t kguess = limit < cnt ? limit : cnt;
    // Enough queries for the scan to be a dense GEMM: bf16 MFMA path with exact re-score; queries
    // whose exactness certificate fails are re-run on the exact single-query path inside it.
    bool use_mfma = e->batch_mode.load() != 0 && (int64_t)nq >= e->batch_min.load() && dims == e->dims &&
                    (dims % 64u) == 0 && cnt > 0 && kguess <= (uint64_t)kBatchMaxK && kguess > 0;
    if (use_mfma && nq < 16) {
        // A small batch costs nq scans of the f32 store on the loop path but ONE pass over the bf16 mirror (half the
        // bytes) plus the fixed pipeline cost on the MFMA path, whatever nq is (measured, profiles/r01/bi_*: 100 K rows
        // 0.15 ms, 1 M rows 0.30 ms, 10 M rows 1.78 ms for any nq <= 16; loop path 0.05 / 0.25 / 2.22 ms PER query).
        // A stale mirror adds its rebuild (read f32, write bf16).
        const double elems = (double)cnt * (double)dims;
        const double t_loop = (double)nq * (elems * 4.0 / 6.9e12 + 25e-6);
        const double t_pass = 135e-6 + elems * 2.0 / 4.7e12;
        const double t_rebuild = mirror_rows_to_convert(e) * (double)dims * 6.0 / 5.0e12;
        use_mfma = t_pass + t_rebuild < t_loop;
        // ... but a steady stream of small batches amortises it: the third one in a row that a valid mirror would have
        // made cheaper pays for the rebuild
        if (!use_mfma && t_pass < t_loop && e->derived.bf16.wanted()) use_mfma = true;
    }
    if (use_mfma) {
        int brc = WAX_HIP_OK;
        bool ran = false;
        {
            DeviceGuard g(e->device);
            ReadGuard rd(e);
            { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return frc; }
            if (e->row_base + e->count > 0x100000000ull)
                return fail(WAX_HIP_ERR_CAPACITY, "row_base + count exceeds UInt32 row indices");
            uint64_t k64 = limit < e->count ? limit : e->count;   // the row count this batch is answered on
            if (k64 > stride) k64 = stride;                       // a smaller result array: the best `stride` of them
            OnepassPlan plan{};
            bool onepass = false;
            if (batch_mfma_applicable(e, dims, (int)k64, nq, &plan, &onepass)) {
                const int k_eff = (int)k64;
                BatchCtx* c = nullptr;
                brc = take_bctx(e, &c);
                if (brc != WAX_HIP_OK) return brc;
                brc = ensure_mirror(e, c->stream);
                if (brc == WAX_HIP_OK) brc = bctx_reserve_host(e, c, nq, (uint64_t)nq * k_eff);
                if (brc == WAX_HIP_OK) {
                    hipError_t err = hipMemcpyAsync(c->d_q, queries, (size_t)nq * dims * sizeof(float), hipMemcpyHostToDevice, c->stream);
                    if (err != hipSuccess) brc = fail(WAX_HIP_ERR_INTERNAL, std::string("query upload: ") + hipGetErrorString(err));
                }
                // The download rides behind the batch's kernels, so the one synchronisation of the finish covers it; only a
                // batch whose rows were rewritten after it (full retries, exact path) downloads again.
                uint32_t rewritten = 0;
                if (brc == WAX_HIP_OK)
                    brc = batch_submit_device_locked(e, c, c->d_q, nq, k_eff, onepass ? &plan : nullptr, c->d_hits, (uint32_t)k_eff);
                if (brc == WAX_HIP_OK) {
                    hipError_t err = hipMemcpyAsync(c->h_hits, c->d_hits, (size_t)nq * k_eff * sizeof(wax_hip_hit), hipMemcpyDeviceToHost, c->stream);
                    if (err != hipSuccess) {
                        (void)hipStreamSynchronize(c->stream);
                        brc = fail(WAX_HIP_ERR_INTERNAL, std::string("hits download: ") + hipGetErrorString(err));
                    }
                }
                if (brc == WAX_HIP_OK)
                    brc = batch_finish_device_locked(e, c, c->d_q, nq, k_eff, c->d_hits, (uint32_t)k_eff, nullptr, &rewritten);
                if (brc == WAX_HIP_OK && rewritten > 0) {
                    hipError_t err = hipMemcpyAsync(c->h_hits, c->d_hits, (size_t)nq * k_eff * sizeof(wax_hip_hit), hipMemcpyDeviceToHost, c->stream);
                    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
                    if (err != hipSuccess) brc = fail(WAX_HIP_ERR_INTERNAL, std::string("hits download: ") + hipGetErrorString(err));
                }
                if (brc == WAX_HIP_OK) {
                    for (uint32_t q = 0; q < nq; ++q) {
                        std::memcpy(out_hits + (size_t)q * stride, c->h_hits + (size_t)q * k_eff, (size_t)k_eff * sizeof(wax_hip_hit));
                        uint32_t m = 0;
                        for (int i = 0; i < k_eff; ++i) m += c->h_hits[(size_t)q * k_eff + i].key != KEY_PAD;
                        out_counts[q] = m;
                    }
                    ran = true;
                } else {
                    (void)hipStreamSynchronize(c->stream);
                }
                e->bctxs.release(c);
            }
        }
        if (brc != WAX_HIP_OK) return brc;
        if (ran) return WAX_HIP_OK;
    }
    // Shared exact passes for batches the MFMA pipelines did not take (top_k beyond the slab pipeline's limit on a store below the
    // one-pass floor, "batch_mode" 0, a batch below "batch_min"): up to 16 queries per pass over the f32 store (scan_multi_kernel: the
    // single-query kernel's arithmetic, bit-identical hits) instead of one scan per query — what the device-resident form has done
    // since round 3. 256 queries at top-100 on a 4 096-row store: 7.9 ms on the loop path below ("batch_host_multi" 0 = that path).
    if (nq >= 16 && dims == e->dims && cnt > 0 && e->batch_host_multi.load() != 0 && e->batch_multi.load() != 0 && e->force_general.load() == 0) {
        int brc = WAX_HIP_OK;
        bool ran = false;
        {
            DeviceGuard g(e->device);
            ReadGuard rd(e);
            { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return frc; }
            if (e->row_base + e->count > 0x100000000ull)
                return fail(WAX_HIP_ERR_CAPACITY, "row_base + count exceeds UInt32 row indices");
            uint64_t k64 = limit < e->count ? limit : e->count;
            if (k64 > stride) k64 = stride;
            if (k64 > 0 && k64 <= (uint64_t)FUSED_MAX_K && scan_multi_group(dims, (int)k64) >= 2) {
                const int k_eff = (int)k64;
                BatchCtx* c = nullptr;
                brc = take_bctx(e, &c);
                if (brc != WAX_HIP_OK) return brc;
                brc = bctx_reserve_host(e, c, nq, (uint64_t)nq * k_eff);
                if (brc == WAX_HIP_OK) {
                    hipError_t err = hipMemcpyAsync(c->d_q, queries, (size_t)nq * dims * sizeof(float), hipMemcpyHostToDevice, c->stream);
                    if (err != hipSuccess) brc = fail(WAX_HIP_ERR_INTERNAL, std::string("query upload: ") + hipGetErrorString(err));
                }
                if (brc == WAX_HIP_OK) {
                    std::vector<uint32_t> all(nq);
                    std::vector<float> norms(nq);
                    for (uint32_t q = 0; q < nq; ++q) {
                        all[q] = q;
                        norms[q] = query_norm(queries + (size_t)q * dims, dims);
                    }
                    brc = exact_scan_queries(e, c, c->d_q, all.data(), norms.data(), nq, k_eff, c->d_hits, (uint32_t)k_eff);   // synchronised on return
                }
                if (brc == WAX_HIP_OK) {
                    hipError_t err = hipMemcpyAsync(c->h_hits, c->d_hits, (size_t)nq * k_eff * sizeof(wax_hip_hit), hipMemcpyDeviceToHost, c->stream);
                    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
                    if (err != hipSuccess) brc = fail(WAX_HIP_ERR_INTERNAL, std::string("hits download: ") + hipGetErrorString(err));
                }
                if (brc == WAX_HIP_OK) {
                    for (uint32_t q = 0; q < nq; ++q) {
                        std::memcpy(out_hits + (size_t)q * stride, c->h_hits + (size_t)q * k_eff, (size_t)k_eff * sizeof(wax_hip_hit));
                        uint32_t m = 0;
                        for (int i = 0; i < k_eff; ++i) m += c->h_hits[(size_t)q * k_eff + i].key != KEY_PAD;
                        out_counts[q] = m;
                    }
                    ran = true;
                } else {
                    (void)hipStreamSynchronize(c->stream);
                }
                e->bctxs.release(c);
            }
        }
        if (brc != WAX_HIP_OK) return brc;
        if (ran) return WAX_HIP_OK;
    }
    // Loop path: pipelined single-query scans over the scratch-slot pool.
    std::vector<uint32_t> todo(nq);
    for (uint32_t q = 0; q < nq; ++q) todo[q] = q;
    const uint32_t depth = (uint32_t)std::max(e->slots.cap(), 1);
    std::vector<uint64_t> tk(todo.size(), 0);
    size_t submitted = 0, collected = 0;
    int rc = WAX_HIP_OK;
    while (collected < todo.size()) {
        while (submitted < todo.size() && submitted - collected < depth) {
            // holding tickets already => never wait for a slot (another batch may be doing the same): collect instead
            rc = submit_impl(e, queries + (uint64_t)todo[submitted] * dims, dims, top_k, &tk[submitted],
                             /*try_only=*/submitted > collected);
            if (rc == kSlotBusy) { rc = WAX_HIP_OK; break; }
            if (rc != WAX_HIP_OK) break;
            ++submitted;
        }
        if (rc != WAX_HIP_OK) break;
        const uint32_t q = todo[collected];
        rc = collect_impl(e, tk[collected], nullptr, nullptr, 0, &out_counts[q], out_hits + (uint64_t)q * stride, stride);
        ++collected;
        if (rc != WAX_HIP_OK) break;
    }
    if (rc != WAX_HIP_OK) {  // drain whatever is still in flight so the shared lock is released
        std::string keep = g_last_error;
        uint32_t dummy = 0;
        std::vector<wax_hip_hit> tmp(stride ? stride : 1);
        for (size_t i = collected; i < submitted; ++i)
            (void)collect_impl(e, tk[i], nullptr, nullptr, 0, &dummy, tmp.data(), stride);
        g_last_error = keep;
    }
    return rc;
}

int wax_hip_search_batch_hits(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k,
                              wax_hip_hit* out_hits, uint32_t out_stride, uint32_t* out_counts) {
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (nq == 0) return WAX_HIP_OK;
    if (!queries || !out_counts || (!out_hits && out_stride)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null input");
    if (e->sh) return sh_search_batch_hits(e, queries, nq, dims, top_k, out_hits, out_stride, out_counts);
    return search_batch_hits_impl(e, queries, nq, dims, top_k, out_hits, out_stride, out_counts);
}

int wax_hip_search_batch(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k,
                         uint64_t* out_ids, float* out_scores, uint32_t out_stride, uint32_t* out_counts) {
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (nq == 0) return WAX_HIP_OK;
    if (!queries || !out_counts) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null input");
    if ((!out_ids || !out_scores) && out_stride) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "output arrays are null");
    const uint32_t limit = (uint32_t)clamp_topk(top_k);
    const uint32_t w = limit < out_stride ? limit : out_stride;          // hits per query worth fetching
    std::vector<wax_hip_hit> hits((size_t)nq * (w ? w : 1));
    int rc = e->sh ? sh_search_batch_hits(e, queries, nq, dims, top_k, hits.data(), w, out_counts)
                   : search_batch_hits_impl(e, queries, nq, dims, top_k, hits.data(), w, out_counts);
    if (rc != WAX_HIP_OK) return rc;
    for (uint32_t q = 0; q < nq; ++q)
        hits_to_results(e->metric, hits.data() + (size_t)q * w, w, out_ids + (uint64_t)q * out_stride,
                        out_scores + (uint64_t)q * out_stride, out_stride, &out_counts[q]);
    return WAX_HIP_OK;
}

// Device-resident form: queries already in HBM (row-major nq x dims f32 on the engine's device), hits left in HBM
// ([nq][out_stride], rows padded). Blocking; `stream` is the stream whose earlier work produced d_queries (the
// library's own stream waits for it), and on return every result is complete. The only PCIe traffic is nq
// certificate flags + norms (8 bytes per query) — or the query block itself when the batch has to take the loop path.
// Shared body of the blocking and the pipelined device-resident batch search. ticket == nullptr: blocking.
// Would wax_hip_search_batch_submit_device on this (single-device) engine finish device work before it returns? True for
// everything but the asynchronous MFMA pipeline with a ready mirror: the loop path (dims not a multiple of 64, k beyond the
// MFMA limits, batch_mode = 0, small nq under the cost model) ends with a stream synchronise, and a mirror (re)build is
// synchronous too. The sharded handle asks before it decides whether ONE thread may drive every shard's submit
// (sharded.inc: sh_batch_submit). Conservative for nq < 16 (the cost model has a side effect; a worker hop costs microseconds).
bool batch_submit_blocks(wax_hip_engine* e, uint32_t dims, int32_t top_k, uint32_t nq, uint32_t out_stride) {
    if (nq == 0 || e->count == 0) return false;
    const uint64_t limit = (uint64_t)clamp_topk(top_k);
    uint64_t k64 = limit < e->count ? limit : e->count;
    if (k64 > out_stride) k64 = out_stride;
    if (k64 == 0) return false;
    OnepassPlan plan{};
    bool onepass = false;
    if ((int64_t)nq < e->batch_min.load() || nq < 16) return true;
    if (!batch_mfma_applicable(e, dims, (int)k64, nq, &plan, &onepass)) return true;
    if (e->pend_rows.load() != 0) return true;               // staged appends are flushed (and the mirror rebuilt) inside submit
    // an incremental conversion (appended / upserted rows) is a small asynchronous launch; (re)allocation and a whole-store conversion are not
    return e->batch.mirror_cap < e->capacity || mirror_rows_to_convert(e) > 65536.0;
}

static int batch_device_impl(wax_hip_engine* e, const float* d_queries, uint32_t nq, uint32_t dims, int32_t top_k,
                             wax_hip_hit* d_out_hits, uint32_t out_stride, void* stream, uint64_t* ticket, const char* what) {
    if (ticket) *ticket = 0;
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    (void)what;
    if (e->sh) return sh_batch_device(e, d_queries, nq, dims, top_k, d_out_hits, out_stride, stream, ticket);   // queries / hits on the handle's first device
    if (nq > 0 && (!d_queries || !d_out_hits || out_stride == 0)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null input");
    if (nq > 0 && dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));
    DeviceGuard g(e->device);
    const bool holder = holding(e) > 0;
    e->lock.lock_shared(holder);
    bool keep_lock = false;   // a pending ticket keeps the shared lock until its collect
    struct Unlock { RWLock& l; bool& keep; ~Unlock() { if (!keep) l.unlock_shared(); } } unlock{e->lock, keep_lock};
    auto done_ticket = [&]() {   // answered (or nothing to do) at submit time: a ticket whose collect is a no-op
        if (ticket) *ticket = e->btickets.put(wax_hip_engine::BatchTicket{});
    };
    if (nq == 0) { done_ticket(); return WAX_HIP_OK; }
    { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return frc; }
    if (e->row_base + e->count > 0x100000000ull) return fail(WAX_HIP_ERR_CAPACITY, "row_base + count exceeds UInt32 row indices");
    const uint64_t limit = (uint64_t)clamp_topk(top_k);
    uint64_t k64 = limit < e->count ? limit : e->count;
    if (k64 > out_stride) k64 = out_stride;
    const int k_eff = (int)k64;
    BatchCtx* c = nullptr;
    int rc = take_bctx(e, &c, /*try_only=*/ticket != nullptr && holder);
    if (rc != WAX_HIP_OK) return rc;
    bool keep_ctx = false;
    struct Release { wax_hip_engine* e; BatchCtx* c; bool& keep; ~Release() { if (!keep) e->bctxs.release(c); } } release{e, c, keep_ctx};
    hipStream_t st = c->stream;
    // inputs are produced on the caller's stream: the workspace's stream waits for what is pending there. A caller stream
    // that has already drained (the usual blocking caller) needs no marker packet on it and no barrier packet in front
    // of the first kernel here ("batch_in_wait" 1 always records + waits, as rounds 1-5 did).
    const bool caller_busy = e->batch_in_wait.load() != 0 || hipStreamQuery(static_cast<hipStream_t>(stream)) != hipSuccess;
    (void)hipGetLastError();   // hipErrorNotReady is an answer, not an error to be found behind the next launch
    if (caller_busy) {
        HIP_TRY(hipEventRecord(c->ev_in, static_cast<hipStream_t>(stream)), WAX_HIP_ERR_INTERNAL, "input event record");
        HIP_TRY(hipStreamWaitEvent(st, c->ev_in, 0), WAX_HIP_ERR_INTERNAL, "input event wait");
    }
    if (k_eff == 0) {   // empty engine: all padding
        std::vector<wax_hip_hit> pad((size_t)nq * out_stride, wax_hip_hit{KEY_PAD, ID_PAD});
        HIP_TRY(hipMemcpyAsync(d_out_hits, pad.data(), pad.size() * sizeof(wax_hip_hit), hipMemcpyHostToDevice, st), WAX_HIP_ERR_INTERNAL, "pad upload");
        HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "pad upload");
        done_ticket();
        return WAX_HIP_OK;
    }
    OnepassPlan plan{};
    bool onepass = false;
    bool use_mfma = (int64_t)nq >= e->batch_min.load() && batch_mfma_applicable(e, dims, k_eff, nq, &plan, &onepass);
    if (use_mfma && nq < 16) {   // same cost model as the host-pointer form
        const double elems = (double)e->count * (double)dims;
        const double t_loop = (double)nq * (elems * 4.0 / 6.9e12 + 25e-6);
        const double t_pass = 135e-6 + elems * 2.0 / 4.7e12;
        const double t_rebuild = mirror_rows_to_convert(e) * (double)dims * 6.0 / 5.0e12;
        use_mfma = t_pass + t_rebuild < t_loop;
        if (!use_mfma && t_pass < t_loop && e->derived.bf16.wanted()) use_mfma = true;
    }
    if (use_mfma) {
        rc = ensure_mirror(e, st);
        if (rc != WAX_HIP_OK) return rc;
        if (!ticket) return batch_search_device_locked(e, c, d_queries, nq, k_eff, onepass ? &plan : nullptr, d_out_hits, out_stride, nullptr);
        rc = batch_submit_device_locked(e, c, d_queries, nq, k_eff, onepass ? &plan : nullptr, d_out_hits, out_stride);
        if (rc != WAX_HIP_OK) return rc;
        wax_hip_engine::BatchTicket t;
        t.c = c; t.d_queries = d_queries; t.d_out = d_out_hits; t.nq = nq; t.out_stride = out_stride; t.k_eff = k_eff;
        e->holders.note_submit(&t.owner);
        *ticket = e->btickets.put(t);
        keep_ctx = true;
        keep_lock = true;
        return WAX_HIP_OK;
    }
    // loop path (batches the MFMA pipelines do not take): exact scans on the workspace's stream — groups of queries
    // share one pass over the f32 store (exact_scan_queries); the norms come from the host
    std::vector<float> hq((size_t)nq * dims);
    HIP_TRY(hipMemcpyAsync(hq.data(), d_queries, hq.size() * sizeof(float), hipMemcpyDeviceToHost, st), WAX_HIP_ERR_INTERNAL, "query download");
    HIP_TRY(hipStreamSynchronize(st), WAX_HIP_ERR_INTERNAL, "query download");
    std::vector<uint32_t> all(nq);
    std::vector<float> norms(nq);
    for (uint32_t q = 0; q < nq; ++q) {
        all[q] = q;
        norms[q] = query_norm(hq.data() + (size_t)q * dims, dims);
    }
    rc = exact_scan_queries(e, c, d_queries, all.data(), norms.data(), nq, k_eff, d_out_hits, out_stride);
    if (rc == WAX_HIP_OK) done_ticket();
    return rc;
}

int wax_hip_search_batch_hits_device(wax_hip_engine* e, const float* d_queries, uint32_t nq, uint32_t dims, int32_t top_k,
                                     wax_hip_hit* d_out_hits, uint32_t out_stride, void* stream) {
    return batch_device_impl(e, d_queries, nq, dims, top_k, d_out_hits, out_stride, stream, nullptr, "wax_hip_search_batch_hits_device");
}

int wax_hip_search_batch_submit_device(wax_hip_engine* e, const float* d_queries, uint32_t nq, uint32_t dims, int32_t top_k,
                                       wax_hip_hit* d_out_hits, uint32_t out_stride, void* stream, uint64_t* out_ticket) {
    if (!out_ticket) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "ticket is null");
    return batch_device_impl(e, d_queries, nq, dims, top_k, d_out_hits, out_stride, stream, out_ticket, "wax_hip_search_batch_submit_device");
}

// out_rewritten (internal; see batch_finish_device_locked): rows of the batch's output written during this call
int batch_collect_device_impl(wax_hip_engine* e, uint64_t ticket, uint32_t* out_fallbacks, uint32_t* out_rewritten) {
    if (out_fallbacks) *out_fallbacks = 0;
    if (out_rewritten) *out_rewritten = 0;
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    if (e->sh) return sh_batch_collect_device(e, ticket, out_fallbacks);
    wax_hip_engine::BatchTicket t;
    if (!e->btickets.take(ticket, &t)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "unknown batch ticket " + std::to_string(ticket));
    if (!t.c) return WAX_HIP_OK;   // answered at submit time
    DeviceGuard g(e->device);
    const int rc = batch_finish_device_locked(e, t.c, t.d_queries, t.nq, t.k_eff, t.d_out, t.out_stride, out_fallbacks, out_rewritten);
    if (rc != WAX_HIP_OK) (void)hipStreamSynchronize(t.c->stream);
    e->bctxs.release(t.c);
    e->holders.note_collect(t.owner);
    e->lock.unlock_shared();
    return rc;
}

int wax_hip_search_batch_collect_device(wax_hip_engine* e, uint64_t ticket, uint32_t* out_fallbacks) {
    return batch_collect_device_impl(e, ticket, out_fallbacks, nullptr);
}

