// api_wide.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: wax_hip_search_wide — one blocking query for k up to MIRROR_WIDE_MAX_K from a mirror pass and the wide finish
// (mirror_wide.hip; DESIGN 4.1, "The wide finish") — and wax_hip_mirror_wide_probe, the finish's selection on made-up lists.

// the hits of the existing search for this call: a ticket, collected in its raw-hit form (k <= MIRROR_MAX_K takes the routes it has)
static int wide_forward(wax_hip_engine* e, const float* query, uint32_t dims, uint32_t top_k, wax_hip_hit* hits_out, uint32_t* count_out) {
    uint64_t t = 0;
    const int rc = submit_impl(e, query, dims, (int32_t)top_k, &t, false);
    if (rc != WAX_HIP_OK) return rc;
    return collect_impl(e, t, nullptr, nullptr, 0, count_out, hits_out, top_k);
}

// A sharded handle answers with its search fan-out. That returns (frame id, score); the hits carry the distance the score stands for
// (VectorMetric.score(fromDistance:) is undone exactly: 1 - (1 - d) == d wherever 1 - d was exact or d came from a rounded 1 - d) and
// the rank in the row word, so wax_hip_hits_to_results gives back search's arrays.
static int wide_sharded(wax_hip_engine* e, const float* query, uint32_t dims, uint32_t top_k, wax_hip_hit* hits_out, uint32_t* count_out) {
    std::vector<uint64_t> ids(top_k);
    std::vector<float> scores(top_k);
    uint32_t n = 0;
    const int rc = wax_hip_search(e, query, dims, (int32_t)top_k, ids.data(), scores.data(), top_k, &n);
    if (rc != WAX_HIP_OK) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        const float d = e->metric == WAX_HIP_METRIC_COSINE ? 1.0f - scores[i] : -scores[i];
        hits_out[i] = wax_hip_hit{make_key(d, i), ids[i]};
    }
    *count_out = n;
    return WAX_HIP_OK;
}

int wax_hip_search_wide(wax_hip_engine* e, const float* query, uint32_t dims, uint32_t top_k, uint32_t bits, wax_hip_hit* hits_out,
                        uint32_t* count_out, uint64_t* stats_out) {
    if (!e || !hits_out || !count_out) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine/hits/count is null");
    if (top_k < 1 || top_k > (uint32_t)MIRROR_WIDE_MAX_K) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "search_wide: top_k is 1 to 1024");
    if (bits != 0 && bits != 8 && bits != 16) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "search_wide: bits is 0, 8 or 16");
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // mirror streamed, certified, m, source of B, lists, C, re-ran on f32, 0
    auto report = [&](int rc) { if (stats_out) std::memcpy(stats_out, stats, sizeof(stats)); return rc; };
    *count_out = 0;
    for (uint32_t i = 0; i < top_k; ++i) hits_out[i] = wax_hip_hit{KEY_PAD, ID_PAD};
    if (e->sh) return report(wide_sharded(e, query, dims, top_k, hits_out, count_out));
    if (top_k <= (uint32_t)MIRROR_MAX_K) return report(wide_forward(e, query, dims, top_k, hits_out, count_out));

    DeviceGuard g(e->device);
    ReadGuard rd(e);
    { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) return report(frc); }
    if (e->count == 0) return report(WAX_HIP_OK);
    if (dims != e->dims || !query) return report(fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, query ? dims : 0)));
    if (e->row_base + e->count > 0x100000000ull) return report(fail(WAX_HIP_ERR_CAPACITY, "row_base + count exceeds UInt32 row indices"));
    const int k_eff = (uint64_t)top_k < e->count ? (int)top_k : (int)e->count;
    Slot* s = nullptr;
    int rc = take_slot(e, &s, false, rd.holder);
    if (rc != WAX_HIP_OK) return report(rc);
    s->k_eff = k_eff; s->timed = false; s->mirror = false; s->mirror8 = false; s->want8 = false; s->flag_wait = false;
    s->shared = false; s->listed = false; s->park_rc = WAX_HIP_OK;
    reset_ticket_extras(s, nullptr, (int32_t)top_k);
    const float qn = query_norm(query, dims);
    // which mirror: the caller's, or (0) the code mirror unless "mirror_bits" is 16 — then by a ticket's own rules (mirror8_take_now:
    // not while the breaker holds, a stale code mirror rebuilt by the third query that wants it). An explicit 8 is the caller's
    // experiment: it asks the breaker nothing and tells it nothing.
    const bool want8 = bits == 8 || (bits == 0 && e->mirror_bits.load() != 16 && mirror8_take_now(e));
    // the shapes and kernel variant a lone mirror pass serves (scan_uses_mirror's, without its size rule: the caller chose the route)
    const bool passes = mirror_scan_supported(e->dims, e->metric) && e->variant.load() <= 0 && e->force_general.load() == 0 &&
                        e->grid_blocks.load() <= SCAN_KWAY_MERGE_GRID;
    bool took = false, certified = false;
    hipError_t err = hipSuccess;
    do {
        if (passes) {
            MirrorScanArgs pass{};
            rc = enqueue_mirror_scan(e, s, query, qn, k_eff, 0, &took, want8, &pass);
            if (rc != WAX_HIP_OK) break;
            if (took) {
                const int c = mirror_wide_candidates(k_eff);
                rc = enqueue_mirror_wide(e, s, pass, c);
                if (rc != WAX_HIP_OK) break;
                if ((err = hipStreamSynchronize(s->stream)) != hipSuccess) break;
                certified = __atomic_load_n(slot_cert_word(s->h_done), __ATOMIC_ACQUIRE) == 1u;
                const uint64_t* r = slot_wide_report(s);
                stats[0] = s->mirror8 ? 8 : 16; stats[1] = certified ? 1 : 0; stats[2] = r[0]; stats[3] = r[1];
                stats[4] = (uint64_t)pass.lists; stats[5] = (uint64_t)c;
                if (s->mirror8 && bits == 0) mirror8_note_result(e, certified);
            }
        }
        if (!certified) {
            // no mirror, or no certificate (ties, a clustered store, a NaN query): the f32 scan on the same slot, and its answer
            if (took) { e->st_mirror_fallbacks++; if (s->mirror8) e->st_mirror8_fallbacks++; }
            else { std::memcpy(s->h_query, query, (size_t)dims * sizeof(float)); s->q_norm = qn; }
            stats[6] = 1;
            // (as a submit: the query rides in the kernel arguments where the fused scan takes it there, else it is uploaded)
            const bool qargs = scan_uses_query_args(e, k_eff, true);
            if (!qargs && (err = hipMemcpyAsync(s->d_query, s->h_query, (size_t)dims * sizeof(float), hipMemcpyHostToDevice, s->stream)) != hipSuccess) break;
            rc = enqueue_scan(e, qargs ? nullptr : s->d_query, s->q_norm, k_eff, k_eff, s->d_partials, s, s->h_hits, s->stream, nullptr, nullptr,
                              /*chain=*/false, nullptr, nullptr, s->h_query);
            if (rc != WAX_HIP_OK) break;
            err = hipStreamSynchronize(s->stream);
        }
    } while (0);
    if (rc == WAX_HIP_OK && err != hipSuccess) rc = fail(WAX_HIP_ERR_INTERNAL, std::string("search_wide failed on device: ") + hipGetErrorString(err));
    if (rc == WAX_HIP_OK) {
        uint32_t n = 0;
        for (int i = 0; i < k_eff; ++i) {
            hits_out[i] = s->h_hits[i];
            n += hits_out[i].key != KEY_PAD;
        }
        *count_out = n;
    } else {
        rearm_slot(s);               // (collect's recovery: a later scan on this slot must not read a half-counted ticket)
    }
    e->slots.release(s);
    return report(rc);
}

int wax_hip_mirror_wide_probe(const int64_t* lists_host, int32_t lists, uint32_t c, int64_t* candidates_out, uint32_t* count_out,
                              int64_t* bound_out, uint32_t* source_out) {
    if (!lists_host || !candidates_out || !count_out || !bound_out || !source_out) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (lists < 1 || lists > SCAN_KWAY_MERGE_GRID) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror_wide_probe: 1 to 512 lists");
    if (c != 1024u && c != (uint32_t)MIRROR_WIDE_MAX_C) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror_wide_probe: c is 1024 or 4096");
    const size_t in_bytes = (size_t)lists * MIRROR_KP * sizeof(int64_t), cand_bytes = (size_t)c * sizeof(int64_t);
    char* d = nullptr;
    HIP_TRY(hipMalloc(&d, in_bytes + cand_bytes + MIRROR_WIDE_CTL * sizeof(uint64_t)), WAX_HIP_ERR_INTERNAL, "mirror_wide_probe allocation");
    int64_t* d_cand = reinterpret_cast<int64_t*>(d + in_bytes);
    uint64_t* d_ctl = reinterpret_cast<uint64_t*>(d + in_bytes + cand_bytes);
    uint64_t ctl[MIRROR_WIDE_CTL] = {};
    hipError_t err = hipMemcpy(d, lists_host, in_bytes, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = launch_mirror_wide_select(reinterpret_cast<const int64_t*>(d), lists, (int)c, d_cand, d_ctl, nullptr);
    if (err == hipSuccess) err = hipMemcpy(candidates_out, d_cand, cand_bytes, hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIP_TRY(err, WAX_HIP_ERR_INTERNAL, "mirror_wide_probe");
    *count_out = (uint32_t)ctl[0];
    *source_out = (uint32_t)ctl[1];
    *bound_out = (int64_t)ctl[2];
    return WAX_HIP_OK;
}
