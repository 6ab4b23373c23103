// search_internal.inc — part of engine.hip's translation unit (included there; not compiled alone).
// one query -> one scan: which launch form a scan takes and how it is enqueued (`enqueue_scan`), hits -> results (MetalVectorEngine.swift:446-627, VectorMetric.swift:32-43)

struct Enqueued { int k_eff; };

// The scan + select chain for one query on `stream`; leaves kpad hits in d_hits.
// Does a scan of this engine for k_eff results take its query through the kernel arguments ("query_args")? Decided BEFORE the
// query would be uploaded: the fused path only (the general selection reads the query through its pointer), the default kernel
// variant, dimensions scan_kernel_qarg exists for.
// Will a scan submitted now run in a stream of scans whose merge is better left to a second launch ("merge_overlap_mb")?
bool scan_overlaps_merge(wax_hip_engine* e, bool others_in_flight) {
    const int64_t mb = e->merge_overlap_mb.load();
    return others_in_flight && mb > 0 && e->count * (uint64_t)e->dims * sizeof(float) >= (uint64_t)mb << 20;
}

bool scan_uses_query_args(wax_hip_engine* e, int k_eff, bool has_general_slot, bool overlap_merge = false) {
    const int64_t mode = e->query_args.load();
    if (mode == 0 || !scan_query_args_dims(e->dims) || k_eff > FUSED_MAX_K) return false;
    if (e->force_general.load() && has_general_slot) return false;
    const int variant = (int)e->variant.load();
    if (variant > 0) return false;
    if (mode >= 2) return true;
    const int grid = scan_grid_for((uint32_t)e->count, e->dims, 0, (int)e->grid_blocks.load());
    if (grid <= SCAN_FUSE_MERGE_GRID) return true;
    // larger stores: where the scan is the query's only packet (it merges in its own kernel: k <= SCAN_KWAY_MAX_K, <= 2 GiB of rows)
    return e->fuse_merge.load() != 0 && !overlap_merge && scan_merges_in_kernel(grid, k_eff, e->merge_kway.load() != 0, (uint32_t)e->count, e->dims);
}

// wave-list capacity of a fused scan that keeps k keys per workgroup (the CAP template argument of the scan and merge kernels)
static inline int wave_list_cap(int k) { return k <= 64 ? 128 : 256; }

// The second-launch merge of `grid` per-workgroup lists of k_eff keys (a fused scan that did not merge in its own kernel; the masked
// scan): kpad hits in d_hits. 64 < k <= 192 (no k-way merge of the heads): the short selection merges the lists first — sorts their
// first few entries and the prefixes below the k-th of those in LDS, ~15 us where the wave-list merge of grid x k keys takes 100 - 350
// (1M rows, top-192, blocking: 0.60 -> 0.3 ms). Lists of k entries cannot have dropped a row of the answer: no certificate; the merge
// kernel stays behind it, gated, for prefixes that overflow the LDS buffer (flag words: the ticket's cache line behind the lists).
// *out_short (if given) = the short selection was enqueued.
int enqueue_list_merge(wax_hip_engine* e, int64_t* d_partials, int grid, int k_eff, int kpad, int cap, uint32_t row_base, uint32_t n_rows,
                       wax_hip_hit* d_hits, hipStream_t stream, bool* out_short) {
    uint32_t* short_flags = nullptr;
    if (e->select_short.load() != 0 && k_eff > SCAN_KWAY_MAX_K && select_short_viable(k_eff, grid, k_eff)) {
        short_flags = partials_ticket(d_partials) + 8;
        HIP_TRY(launch_select_short(d_partials, (uint32_t)grid, (uint32_t)k_eff, k_eff, kpad, e->d_ids, row_base, n_rows, short_flags, d_hits, stream),
                WAX_HIP_ERR_INTERNAL, "short merge launch");
    }
    if (out_short) *out_short = short_flags != nullptr;
    HIP_TRY(launch_merge_keys(d_partials, (uint32_t)grid * (uint32_t)k_eff, k_eff, kpad, e->d_ids, row_base, n_rows, d_hits, cap, stream, short_flags),
            WAX_HIP_ERR_INTERNAL, "merge kernel launch");
    return WAX_HIP_OK;
}

// d_query == nullptr: the query is `h_query` (host memory, read during this call) and travels in the kernel arguments.
int enqueue_scan(wax_hip_engine* e, const float* d_query, float q_norm, int k_eff, int kpad, int64_t* d_partials,
                 Slot* general_slot, wax_hip_hit* d_hits, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1,
                 bool chain = false, hipEvent_t* used_start = nullptr, hipEvent_t* used_end = nullptr,
                 const float* h_query = nullptr, uint64_t* done_flag = nullptr, uint64_t done_value = 0, bool* out_flagged = nullptr,
                 bool overlap_merge = false, int tk_mode = 0) {
    // tk_mode: the caller's ONE read of "time_kernels" for this submit (a concurrent set_tuning between two reads could otherwise arm
    // ev0 / ev1 one way and mark the slot as timed the other: advisor, round 5)
    ScanArgs a{};
    a.store = e->d_store;
    a.query = d_query;
    a.query_host = d_query == nullptr ? h_query : nullptr;
    a.done_flag = done_flag;
    a.done_value = done_value;
    a.no_kway = e->merge_kway.load() != 0 ? 0 : 1;
    {
        // ordinary (cacheable) instead of non-temporal row loads: "scan_plain_mb" = stores of at most N MB (default 32); -1 = stores whose
        // grid fits the wave-list fused merge (<= 160 workgroups). Measured on one box (profiles/r04/n_latency_small_stores_*): ordinary loads
        // are 0.7-0.9 us per query faster at 5K / 10K / 20K rows x 384 (7.7 / 15 / 31 MB), equal from 60 to 230 MB, 10 % slower beyond.
        // (FETCH_SIZE still shows the whole store crossing the L2 -> fabric boundary on every query: the gain is on the memory side.)
        const int64_t mb = e->scan_plain_mb.load();
        a.plain_loads = mb < 0 ? (scan_grid_for((uint32_t)e->count, e->dims, 0, (int)e->grid_blocks.load()) <= SCAN_FUSE_MERGE_GRID)
                               : ((uint64_t)e->count * e->dims * sizeof(float) <= (uint64_t)mb << 20);
    }
    if (out_flagged) *out_flagged = false;
    a.partials = d_partials;
    a.dist_out = nullptr;
    a.n_rows = (uint32_t)e->count;
    a.row_base = (uint32_t)e->row_base;
    a.dims = e->dims;
    a.k = k_eff;
    a.q_norm = q_norm;
    const bool fused = k_eff <= FUSED_MAX_K && !(e->force_general.load() && general_slot != nullptr);
    int grid = 0;
    std::unique_lock<std::mutex> chain_guard(e->chain_mu, std::defer_lock);
    if (chain) {
        chain_guard.lock();
        if (e->scan_done_valid) HIP_TRY(hipStreamWaitEvent(stream, e->chain_event, 0), WAX_HIP_ERR_INTERNAL, "scan chain wait");
    }
    if (used_start) *used_start = ev0;
    if (used_end) *used_end = ev1;
    // "time_kernels" = 2: the event pair is bound to the scan's dispatch itself (kernels.h: launch_kernel) — no trailing marker and no
    // chain wait inside the interval; 1: the pair is recorded in front of and behind the launch.
    const bool bound = ev0 != nullptr && ev1 != nullptr && tk_mode == 2;
    if (fused) {
        const int cap = wave_list_cap(k_eff);
        bool record_start = ev0 != nullptr && !bound;
        if (!bound && chain_guard.owns_lock() && ev0 && ev1 && used_start && used_end && e->share_timing.load() != 0) {
            hipEvent_t& slot_ev = e->tev[e->tev_next % wax_hip_engine::kTimingRing];
            if (!slot_ev && hipEventCreateWithFlags(&slot_ev, hipEventReleaseToDevice) != hipSuccess) slot_ev = nullptr;
            if (slot_ev) {
                ++e->tev_next;
                ev1 = slot_ev;
                // previous scan still in flight: this one starts when that one ends, and that moment is already recorded
                if (e->scan_done_valid && e->chain_is_timing && hipEventQuery(e->chain_event) == hipErrorNotReady) {
                    ev0 = e->chain_event;
                    record_start = false;
                }
                *used_start = ev0;
                *used_end = ev1;
            }
        }
        if (record_start) HIP_TRY(hipEventRecord(ev0, stream), WAX_HIP_ERR_INTERNAL, "event record");
        // small grids: the last-arriving workgroup does the final merge itself (one launch per query instead of two)
        bool merged = false;
        // (overlap_merge: a large store in a stream of scans — the merge launch behind this scan overlaps the next one)
        const bool small_grid = scan_grid_for((uint32_t)e->count, e->dims, 0, (int)e->grid_blocks.load()) <= SCAN_FUSE_MERGE_GRID;
        if (e->fuse_merge.load() != 0 && (!overlap_merge || small_grid)) { a.merge_out = d_hits; a.ids = e->d_ids; a.arrive = partials_ticket(d_partials); a.kpad = kpad; }
        else if (overlap_merge) e->st_overlap_scans++;
        if (bound) launch_timing() = LaunchTiming{ev0, ev1};
        const hipError_t lerr = launch_scan(a, e->metric, (int)e->variant.load(), cap, false, (int)e->grid_blocks.load(), stream, &grid, &merged);
        launch_timing() = LaunchTiming{};
        HIP_TRY(lerr, WAX_HIP_ERR_INTERNAL, "scan kernel launch");
        if (ev1 && !bound) HIP_TRY(hipEventRecord(ev1, stream), WAX_HIP_ERR_INTERNAL, "event record");
        if (chain_guard.owns_lock()) {
            // the next scan (on the other stream) starts when this one ends: its end-of-kernel timing event doubles
            // as the chain event when kernels are timed — every packet between two scans costs microseconds
            // (kernel-bound timing: the packets between two scans are outside the interval, so the chain has its own event)
            if (ev1 && !bound) {
                e->chain_event = ev1;
                e->chain_is_timing = true;
            } else {
                HIP_TRY(hipEventRecord(e->scan_done, stream), WAX_HIP_ERR_INTERNAL, "scan chain record");
                e->chain_event = e->scan_done;
                e->chain_is_timing = false;
            }
            e->scan_done_valid = true;
            chain_guard.unlock();
        }
        if (merged) e->st_merged_scans++;
        if (out_flagged) *out_flagged = merged && done_flag != nullptr;   // the kernel itself publishes the completion word
        if (!merged) {
            bool short_selected = false;
            const int mrc = enqueue_list_merge(e, d_partials, grid, k_eff, kpad, cap, a.row_base, a.n_rows, d_hits, stream, &short_selected);
            if (mrc != WAX_HIP_OK) return mrc;
            if (short_selected) e->st_short_selects++;
        }
    } else {
        if (!general_slot) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "top_k too large for the device-resident shard path (max 192)");
        int rc = ensure_general(e, general_slot);
        if (rc != WAX_HIP_OK) return rc;
        // Short selection ("select_short", default 1): the fused scan with FUSED_MAX_K-entry lists per workgroup, ONE selecting
        // workgroup over those lists, and a certificate that no workgroup dropped one of the k best (launch_select_short). The
        // distance pass and the 11-launch radix selection still follow, gated on the certificate's word: they return at once
        // unless it failed (best rows bunched in one workgroup's share: more than 192 of the k best in 1/grid of the rows). Tried
        // only when the lists can hold the answer with room to spare (select_short_viable).
        const int fgrid = scan_grid_for((uint32_t)e->count, e->dims, 0, (int)e->grid_blocks.load());
        // (and only on stores of at least 256 rows per wanted key: below, the radix passes over so few distances cost less than keeping
        // 192-entry lists in the scan and sorting thousands of keys in one workgroup — 100K rows, top-4096: 0.092 ms long, 0.133 short)
        // Lists of 64 (the k <= 64 scan: lighter wave lists, no long rank-merge at the end of every workgroup — alone it takes 2.18 ms
        // at 10M rows where the 192-entry form takes 2.7) while a list holds at most 8 keys of the answer on average; 192 beyond
        // ("select_short" 2 = always 192, for A/B).
        const int64_t ss_mode = e->select_short.load();
        const int per_list = (ss_mode != 2 && (int64_t)k_eff <= (int64_t)fgrid * 8) ? SCAN_KWAY_MAX_K : FUSED_MAX_K;
        const bool try_short = ss_mode != 0 && e->force_general.load() == 0 && select_short_viable(k_eff, fgrid, per_list) && k_eff > FUSED_MAX_K &&
                               e->count >= (uint64_t)k_eff * 256ull;
        if (ev0 && !bound) HIP_TRY(hipEventRecord(ev0, stream), WAX_HIP_ERR_INTERNAL, "event record");
        if (try_short) {
            ScanArgs f = a;
            f.k = per_list; f.kpad = per_list; f.merge_out = nullptr; f.arrive = nullptr; f.done_flag = nullptr; f.query_host = nullptr;
            int lists = 0;
            if (bound) launch_timing() = LaunchTiming{ev0, ev1};
            const hipError_t ferr = launch_scan(f, e->metric, 0, wave_list_cap(per_list), false, (int)e->grid_blocks.load(), stream, &lists);
            launch_timing() = LaunchTiming{};
            HIP_TRY(ferr, WAX_HIP_ERR_INTERNAL, "scan kernel launch");
            if (ev1 && !bound) HIP_TRY(hipEventRecord(ev1, stream), WAX_HIP_ERR_INTERNAL, "event record");
            HIP_TRY(launch_select_short(d_partials, (uint32_t)lists, (uint32_t)per_list, k_eff, kpad, e->d_ids, a.row_base, a.n_rows,
                                        general_slot->sw.flags, d_hits, stream),
                    WAX_HIP_ERR_INTERNAL, "short selection launch");
            e->st_short_selects++;
            a.gate = general_slot->sw.flags;
        }
        a.dist_out = general_slot->d_dist;
        if (bound && !try_short) launch_timing() = LaunchTiming{ev0, ev1};
        const hipError_t lerr = launch_scan(a, e->metric, 0, 128, true, (int)e->grid_blocks.load(), stream, &grid);
        launch_timing() = LaunchTiming{};
        HIP_TRY(lerr, WAX_HIP_ERR_INTERNAL, "distance kernel launch");
        if (try_short) { ev1 = nullptr; }   // (recorded behind the first scan)
        if (ev1 && !bound) HIP_TRY(hipEventRecord(ev1, stream), WAX_HIP_ERR_INTERNAL, "event record");
        if (chain_guard.owns_lock()) {
            // chained scans (a timed calibration pass): the next distance pass starts when this one ends, like the fused scans above —
            // until round 6 this branch left the chain where the last FUSED scan had put it, so two distance passes overlapped and
            // each was "timed" at twice its length
            if (ev1 && !bound) {
                e->chain_event = ev1;
                e->chain_is_timing = true;
            } else {
                HIP_TRY(hipEventRecord(e->scan_done, stream), WAX_HIP_ERR_INTERNAL, "scan chain record");
                e->chain_event = e->scan_done;
                e->chain_is_timing = false;
            }
            e->scan_done_valid = true;
            chain_guard.unlock();
        }
        HIP_TRY(launch_select_general(general_slot->d_dist, a.n_rows, a.row_base, k_eff, kpad, e->d_ids,
                                      general_slot->sw, d_hits, stream, a.gate, (int)e->select_grid.load()),
                WAX_HIP_ERR_INTERNAL, "select kernel launch");
    }
    e->st_searches++;
    e->st_rows += e->count;
    e->st_bytes += e->count * (uint64_t)e->dims * 4ull;
    return WAX_HIP_OK;
}

int hits_to_results(uint8_t metric, const wax_hip_hit* hits, uint32_t n, uint64_t* out_ids, float* out_scores,
                    uint32_t capacity, uint32_t* out_count) {
    uint32_t m = 0;
    for (uint32_t i = 0; i < n && m < capacity; ++i) {
        if (hits[i].key == KEY_PAD) continue;                    // idx == UInt32.max (:597)
        const float d = key_distance(hits[i].key);
        if (!std::isfinite(d)) continue;                         // !distance.isFinite (:597)
        if (hits[i].frame_id == ID_PAD) continue;                // index >= frameIds.count (:599)
        out_ids[m] = hits[i].frame_id;
        // VectorMetric.score(fromDistance:) (VectorMetric.swift:32-43)
        out_scores[m] = (metric == WAX_HIP_METRIC_COSINE) ? (1.0f - d) : (-d);
        ++m;
    }
    *out_count = m;
    return WAX_HIP_OK;
}

// Fold a finished shard-path scan's event pair into the kernel-time statistics.
void harvest_ring_event(wax_hip_engine* e, int r) {
    std::unique_lock<std::mutex> sg(e->st_mu);
    if (!e->ring_ev_pending[r]) return;
    e->ring_ev_pending[r] = false;
    float ms = 0.f;
    if (e->ring_t0[r] && e->ring_t1[r] && hipEventSynchronize(e->ring_t1[r]) == hipSuccess &&
        hipEventElapsedTime(&ms, e->ring_t0[r], e->ring_t1[r]) == hipSuccess) {
        e->st_last_ms = ms; e->st_total_ms += ms; e->st_timed += 1;
    }
}



// ---- one query on the bf16 mirror (mirror_scan.hip; DESIGN 4.1) ----------------------------------------------------------------
int ensure_mirror(wax_hip_engine* e, hipStream_t st);   // batch_host.inc

// chain single-query scans of different streams through an event ("scan_chain"; -1 = while kernels are timed)
static bool chain_scans(wax_hip_engine* e, int tk_mode) {
    const int64_t sc = e->scan_chain.load();
    return sc > 0 || (sc < 0 && tk_mode != 0);
}

// Does a single query of this engine for k_eff results stream the bf16 mirror ("scan_mirror")? Shapes mirror_scan.hip has kernels
// for, the default kernel variant, the fused path's k; in auto mode only stores above the one-launch boundary (SCAN_KWAY_MAX_BYTES:
// below it a scan is latency-bound and merges in its own kernel, above it the f32 scan is bound by HBM bandwidth alone).
bool scan_uses_mirror(wax_hip_engine* e, int k_eff) {
    const int64_t mode = e->scan_mirror.load();
    if (mode == 0 || k_eff < 1 || k_eff > MIRROR_MAX_K || !mirror_scan_supported(e->dims, e->metric)) return false;
    if (e->variant.load() > 0 || e->force_general.load() != 0) return false;
    if (e->grid_blocks.load() > SCAN_KWAY_MERGE_GRID) return false;
    return mode >= 2 || e->count * (uint64_t)e->dims * sizeof(float) > SCAN_KWAY_MAX_BYTES;
}

// ---- which mirror ("mirror_bits"; DESIGN 4.1, "Eight bits per element") ----
int ensure_mirror8(wax_hip_engine* e, hipStream_t st);   // batch_host.inc

// May a single query of this engine that takes a mirror take the 8-bit code mirror? k <= MIRROR8_MAX_K, and either "mirror_bits" 8 or
// auto mode on a store above the one-launch boundary ("scan_mirror" 2 with "mirror_bits" 0 stays bf16: forced small stores keep their path).
static bool mirror8_eligible(wax_hip_engine* e, int k_eff) {
    if (k_eff > MIRROR8_MAX_K) return false;
    const int64_t bits = e->mirror_bits.load();
    if (bits == 16) return false;
    if (bits == 8) return true;
    return e->scan_mirror.load() == 1 && e->count * (uint64_t)e->dims * sizeof(float) > SCAN_KWAY_MAX_BYTES;
}

// The decision for one eligible query, made once at its submit (it counts): not while the breaker holds; at once on a code mirror that
// is valid or only lacks appended rows; a stale or missing one is rebuilt by the third query in a row since the last mutation that
// wanted it — the first two take bf16.
static bool mirror8_take(wax_hip_engine* e, int k_eff) {
    if (!mirror8_eligible(e, k_eff)) return false;
    {
        std::unique_lock<std::mutex> bg(e->breaker_mu);
        if (e->breaker_hold > 0) { --e->breaker_hold; return false; }
    }
    BatchMirror& b = e->batch;
    if (b.c8_cap >= e->capacity && b.d_c8 != nullptr && (e->derived.codes.current() || !e->derived.codes.restarting())) return true;
    return e->derived.codes.wanted();
}

// The certificate of a collected 8-bit query feeds the breaker: kBreakerFails uncertified among the last kBreakerWindow send the next
// kBreakerHold eligible queries to bf16, then the window starts again.
static void mirror8_note_result(wax_hip_engine* e, bool certified) {
    std::unique_lock<std::mutex> bg(e->breaker_mu);
    e->breaker_bits = (e->breaker_bits << 1) | (certified ? 0u : 1u);
    static_assert(kBreakerWindow == 32, "the window is one 32-bit word");
    if (__builtin_popcount(e->breaker_bits) >= kBreakerFails) {
        e->breaker_bits = 0;
        e->breaker_hold = kBreakerHold;
        e->st_mirror8_breaker_trips++;
    }
}

// the code mirror for a launch on `st`: false = it could not be prepared (allocation, conversion launch) and the launch takes bf16
static bool mirror8_ready(wax_hip_engine* e, hipStream_t st, uint64_t nq) {
    const std::string keep = g_last_error;
    BatchMirror& b = e->batch;
    if (ensure_mirror8(e, st) == WAX_HIP_OK && b.d_c8 != nullptr && b.d_c8_meta != nullptr && b.d_c8_max != nullptr) return true;
    (void)hipGetLastError();
    g_last_error = keep;
    e->st_mirror8_unavailable += nq;
    return false;
}

// Enqueue the mirror scan + finish of one query on the slot's stream (the kpad hits and the certificate word land in the slot's pinned
// memory). *took = false: the mirror could not be prepared (allocation, conversion launch) and nothing was enqueued — the caller takes
// the f32 scan; a query never fails because of the mirror. Same chain and timing semantics as the fused f32 branch of enqueue_scan:
// "time_kernels" 2 binds the event pair to the mirror_scan_kernel dispatch, 1 brackets the two launches.
int enqueue_mirror_scan(wax_hip_engine* e, Slot* s, const float* query, float q_norm, int k_eff, int tk_mode, bool* took, bool want8 = false) {
    *took = false;
    BatchMirror& b = e->batch;
    const bool use8 = want8 && mirror8_ready(e, s->stream, 1);
    if (!use8) {
        const std::string keep = g_last_error;
        if (ensure_mirror(e, s->stream) != WAX_HIP_OK || b.d_cb == nullptr || b.d_maxnorm == nullptr) {
            (void)hipGetLastError();                      // a refused allocation must not surface in the f32 launch behind it
            g_last_error = keep;
            e->st_mirror_unavailable++;
            return WAX_HIP_OK;
        }
    }
    if (query != s->h_query) std::memcpy(s->h_query, query, (size_t)e->dims * sizeof(float));   // for the f32 re-run at collect, if the certificate fails (a parked query is there already)
    s->q_norm = q_norm;
    MirrorScanArgs m{};
    m.mirror = b.d_cb;
    m.store = e->d_store;
    m.partials = s->d_partials;
    m.ids = e->d_ids;
    m.hits = s->h_hits;
    m.certified = slot_cert_word(s->h_done);
    m.max_bits = use8 ? b.d_c8_max : b.d_maxnorm;
    m.n_rows = (uint32_t)e->count;
    m.row_base = (uint32_t)e->row_base;
    m.dims = e->dims;
    m.k = k_eff;
    m.kpad = k_eff;
    m.q_norm = q_norm;
    m.use_measured = e->batch_eps_measured.load() != 0 ? 1 : 0;
    hipEvent_t ev0 = s->timed ? s->ev0 : nullptr, ev1 = s->timed ? s->ev1 : nullptr;
    const bool bound = ev0 != nullptr && ev1 != nullptr && tk_mode == 2;
    s->t_start = ev0;
    s->t_end = ev1;
    std::unique_lock<std::mutex> chain_guard(e->chain_mu, std::defer_lock);
    if (chain_scans(e, tk_mode)) {
        chain_guard.lock();
        if (e->scan_done_valid) HIP_TRY(hipStreamWaitEvent(s->stream, e->chain_event, 0), WAX_HIP_ERR_INTERNAL, "scan chain wait");
    }
    if (ev0 && !bound) HIP_TRY(hipEventRecord(ev0, s->stream), WAX_HIP_ERR_INTERNAL, "event record");
    if (bound) launch_timing() = LaunchTiming{ev0, ev1};
    if (use8) m.mirror = nullptr;
    const hipError_t lerr = use8 ? launch_mirror8_scan(m, b.d_c8, b.d_c8_meta, query, e->metric, (int)e->grid_blocks.load(), s->stream)
                                 : launch_mirror_scan(m, query, e->metric, (int)e->grid_blocks.load(), s->stream);
    launch_timing() = LaunchTiming{};
    HIP_TRY(lerr, WAX_HIP_ERR_INTERNAL, "mirror scan launch");
    if (ev1 && !bound) HIP_TRY(hipEventRecord(ev1, s->stream), WAX_HIP_ERR_INTERNAL, "event record");
    if (chain_guard.owns_lock()) {
        HIP_TRY(hipEventRecord(e->scan_done, s->stream), WAX_HIP_ERR_INTERNAL, "scan chain record");
        e->chain_event = e->scan_done;
        e->chain_is_timing = false;
        e->scan_done_valid = true;
        chain_guard.unlock();
    }
    *took = true;
    s->mirror = true;
    s->mirror8 = use8;
    e->st_mirror_scans++;
    e->st_mirror_passes++;
    if (use8) e->st_mirror8_passes++;
    e->st_searches++;
    e->st_rows += e->count;
    e->st_bytes += e->count * (use8 ? (uint64_t)e->dims + 8ull : (uint64_t)e->dims * 2ull) + (uint64_t)MIRROR_KP * e->dims * 4ull;
    return WAX_HIP_OK;
}

// ---- single queries in flight share a pass over the mirror ("mirror_share"; DESIGN 4.1) ----------------------------------------
// A parked ticket holds its slot, the read lock and its query (the slot's pinned h_query) like every ticket; what it lacks is a launch.
// Everything below runs under e->share_mu, on whichever thread got there first.

// May this submit be parked or share a pass? Not while kernels are timed or scans are chained: calibration passes stay one kernel
// per query.
static int64_t mirror_share_mode(wax_hip_engine* e, int tk_mode) {
    if (tk_mode != 0 || chain_scans(e, tk_mode)) return 0;
    return e->mirror_share.load();
}

// the f32 scan of a parked query on its own slot and stream (the mirror could not be prepared)
static int parked_take_f32(wax_hip_engine* e, Slot* s) {
    s->mirror = false;
    s->mirror8 = false;
    const int rc = enqueue_scan(e, nullptr, s->q_norm, s->k_eff, s->k_eff, s->d_partials, s, s->h_hits, s->stream, nullptr, nullptr,
                                /*chain=*/false, nullptr, nullptr, s->h_query);
    if (rc != WAX_HIP_OK) return rc;
    HIP_TRY(hipEventRecord(s->ev_done, s->stream), WAX_HIP_ERR_INTERNAL, "event record");
    return WAX_HIP_OK;
}

// ---- predicate tickets: the bitmap entries (wax_hip_search_predicate_submit; DESIGN 4.5) ---------------------------------------
}  // namespace
static int ensure_attrs(wax_hip_engine* e, hipStream_t st, const int64_t** d_ts, const uint32_t** d_flags);   // api_predicate.inc (file scope, like every api_*.inc)
namespace {

static inline bool same_predicate(const wax_hip_row_predicate& a, const wax_hip_row_predicate& b) {   // both normalised
    return a.has_after == b.has_after && a.after == b.after && a.has_before == b.has_before && a.before == b.before && a.deny_flags == b.deny_flags;
}

// A use of the entry of `np` (normalised) on the store as it is (shared lock held: the epoch stands still): the entry that has it, or
// one without a user — never assigned first, else the least recently used — that the first pass will build. -1: all four are in use.
static int pred_entry_acquire(wax_hip_engine* e, const wax_hip_row_predicate& np) {
    std::unique_lock<std::mutex> g(e->pred_mu);
    const uint64_t epoch = e->lock.epoch();
    int victim = -1;
    for (int i = 0; i < kPredEntries; ++i) {
        PredEntry& p = e->pred_entries[i];
        if (p.assigned && p.epoch == epoch && same_predicate(p.pred, np)) {
            p.users++;
            p.last_use = ++e->pred_tick;
            e->pt_bitmap_hits++;
            return i;
        }
        if (p.users != 0) continue;
        if (victim < 0 || (!p.assigned && e->pred_entries[victim].assigned) ||
            (p.assigned == e->pred_entries[victim].assigned && p.last_use < e->pred_entries[victim].last_use))
            victim = i;
    }
    if (victim < 0) return -1;
    PredEntry& p = e->pred_entries[victim];
    p.pred = np; p.epoch = epoch; p.assigned = true; p.built = false; p.users = 1; p.last_use = ++e->pred_tick;
    return victim;
}

static void pred_entry_release(wax_hip_engine* e, int idx) {
    if (idx < 0) return;
    std::unique_lock<std::mutex> g(e->pred_mu);
    if (e->pred_entries[idx].users > 0) e->pred_entries[idx].users--;
}

// The entry's counts — passing rows, 16-row tiles that hold one — once they have reached the host. wait: block until they have (a
// collect behind the pass finds them there); otherwise false while the build is not enqueued or still running.
static bool pred_entry_counts(wax_hip_engine* e, int idx, bool wait, uint64_t* passing, uint64_t* tiles) {
    std::unique_lock<std::mutex> g(e->pred_mu);
    PredEntry& p = e->pred_entries[idx];
    if (!p.built) return false;
    if (wait) { if (hipEventSynchronize(p.built_ev) != hipSuccess) return false; }
    else if (hipEventQuery(p.built_ev) != hipSuccess) { (void)hipGetLastError(); return false; }
    *passing = p.h_counts[0];
    *tiles = p.h_counts[1];
    return true;
}

// The entry's bitmap for a pass on `st`: built there, in front of the pass, by the first pass that needs it (attribute columns,
// attr_mask_kernel, the counts on their way to pinned memory, an event — no host synchronisation); a pass on another stream waits
// for that event.
static int pred_entry_prepare(wax_hip_engine* e, int idx, hipStream_t st, const uint32_t** bitmap) {
    std::unique_lock<std::mutex> g(e->pred_mu);
    PredEntry& p = e->pred_entries[idx];
    if (!p.built) {
        const uint32_t count = (uint32_t)e->count;
        const uint64_t n_words = ((uint64_t)count + 31) / 32;
        if (p.words < n_words) {             // (no user but this pass's members: nothing reads the old words)
            const uint64_t cap = ((e->capacity > e->count ? e->capacity : e->count) + 31) / 32;
            (void)hipFree(p.d_bitmap);
            p.d_bitmap = nullptr; p.words = 0;
            HIP_TRY(hipMalloc(&p.d_bitmap, (size_t)cap * sizeof(uint32_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate row bitmap");
            p.words = cap;
        }
        if (!p.d_counts) HIP_TRY(hipMalloc(&p.d_counts, kPredCounts * sizeof(uint32_t)), WAX_HIP_ERR_ALLOC, "Failed to allocate predicate counters");
        if (!p.h_counts) HIP_TRY(hipHostMalloc(&p.h_counts, kPredCounts * sizeof(uint32_t), hipHostMallocDefault), WAX_HIP_ERR_ALLOC, "Failed to allocate predicate counters");
        if (!p.built_ev) HIP_TRY(hipEventCreateWithFlags(&p.built_ev, hipEventDisableTiming), WAX_HIP_ERR_ALLOC, "Failed to allocate event");
        const int64_t* d_ts = nullptr;
        const uint32_t* d_fl = nullptr;
        { const int arc = ensure_attrs(e, st, &d_ts, &d_fl); if (arc != WAX_HIP_OK) return arc; }
        AttrMaskArgs ma{};
        ma.ts = d_ts; ma.flags = d_fl; ma.bitmap = p.d_bitmap; ma.counts = p.d_counts; ma.n_rows = count; ma.chunk_rows = 16; ma.chunk_rows2 = 0; ma.and_bitmap = 0;
        ma.has_after = p.pred.has_after != 0; ma.has_before = p.pred.has_before != 0; ma.after = p.pred.after; ma.before = p.pred.before; ma.deny_flags = p.pred.deny_flags;
        HIP_TRY(hipMemsetAsync(p.d_counts, 0, kPredCounts * sizeof(uint32_t), st), WAX_HIP_ERR_INTERNAL, "predicate counters");
        HIP_TRY(launch_attr_mask(ma, st), WAX_HIP_ERR_INTERNAL, "attribute mask launch");
        HIP_TRY(hipMemcpyAsync(p.h_counts, p.d_counts, kPredCounts * sizeof(uint32_t), hipMemcpyDeviceToHost, st), WAX_HIP_ERR_INTERNAL, "row count download");
        HIP_TRY(hipEventRecord(p.built_ev, st), WAX_HIP_ERR_INTERNAL, "event record");
        p.built = true;
        p.build_stream = st;
        e->pt_bitmap_builds++;
    } else if (p.build_stream != st) {
        HIP_TRY(hipStreamWaitEvent(st, p.built_ev, 0), WAX_HIP_ERR_INTERNAL, "bitmap wait");
    }
    *bitmap = p.d_bitmap;
    return WAX_HIP_OK;
}

// a parked or just submitted predicate ticket that cannot ride after all: the blocking body answers it at collect
static void pred_ticket_defer(wax_hip_engine* e, Slot* s) {
    s->pred_deferred = true;
    s->mirror = false;
    s->mirror8 = false;
    e->pt_deferred++;
}

// One pass for `nq` parked queries on the first one's stream: one launch that copies the members' queries from their pinned
// h_query into their d_query (a hipMemcpyAsync per member cost the host as much as a launch each, in the gap in front of the scan),
// the group scan, one finish workgroup per member, and every member's ev_done behind the finish launch. nq >= 2 — or a set with a
// predicate ticket in it, of any size from 1: then the pass is the masked 8-bit one (unmasked members pass a null bitmap), the
// bitmaps are built or waited for in front of it, and the caller has made sure of the code mirror (use8_hint = 1).
static int enqueue_mirror_group(wax_hip_engine* e, Slot* const* grp, int nq, bool* took, int use8_hint = -1) {
    *took = false;
    BatchMirror& b = e->batch;
    hipStream_t st = grp[0]->stream;
    int n_masked = 0;
    for (int i = 0; i < nq; ++i) n_masked += grp[i]->has_pred ? 1 : 0;
    bool use8 = use8_hint >= 0 ? use8_hint != 0 : true;   // one mirror per set: bf16 as soon as one member cannot ride the code mirror (k, breaker, rebuild count)
    if (use8_hint < 0) {
        for (int i = 0; i < nq; ++i) use8 = use8 && grp[i]->want8;
        use8 = use8 && mirror8_ready(e, st, (uint64_t)nq);
    }
    if (n_masked != 0 && !use8) return fail(WAX_HIP_ERR_INTERNAL, "a masked pass needs the code mirror");
    if (!use8) {
        const std::string keep = g_last_error;
        if (ensure_mirror(e, st) != WAX_HIP_OK || b.d_cb == nullptr || b.d_maxnorm == nullptr) {
            (void)hipGetLastError();
            g_last_error = keep;
            e->st_mirror_unavailable += (uint64_t)nq;
            return WAX_HIP_OK;
        }
    }
    MirrorGroupArgs g{};
    g.a.mirror = b.d_cb;
    g.a.store = e->d_store;
    g.a.ids = e->d_ids;
    g.a.max_bits = use8 ? b.d_c8_max : b.d_maxnorm;
    if (use8) g.a.mirror = nullptr;
    g.a.n_rows = (uint32_t)e->count;
    g.a.row_base = (uint32_t)e->row_base;
    g.a.dims = e->dims;
    g.a.use_measured = e->batch_eps_measured.load() != 0 ? 1 : 0;
    MirrorQueryCopies qc{};
    qc.dims = e->dims;
    int one_entry = -1;                    // the entry every member reads, if there is one such (the accounting below)
    bool one = n_masked == nq;
    for (int i = 0; i < nq; ++i) {
        Slot* s = grp[i];
        qc.src[i] = s->h_query;
        qc.dst[i] = s->d_query;
        g.m[i].query = s->d_query;
        g.m[i].partials = s->d_partials;
        g.m[i].hits = s->h_hits;
        g.m[i].certified = slot_cert_word(s->h_done);
        g.m[i].bitmap = nullptr;
        g.m[i].q_norm = s->q_norm;
        g.m[i].k = s->k_eff;
        g.m[i].kpad = s->k_eff;
        s->t_start = nullptr;
        s->t_end = nullptr;
        if (s->has_pred) {
            const int prc = pred_entry_prepare(e, s->pred_entry, st, &g.m[i].bitmap);
            if (prc != WAX_HIP_OK) return prc;
            if (one_entry < 0) one_entry = s->pred_entry;
            else if (one_entry != s->pred_entry) one = false;
        }
    }
    HIP_TRY(launch_mirror_group_queries(qc, nq, st), WAX_HIP_ERR_INTERNAL, "query upload");
    if (n_masked != 0)
        HIP_TRY(launch_mirror8_group_masked(g, b.d_c8, b.d_c8_meta, nq, e->metric, (int)e->grid_blocks.load(), st), WAX_HIP_ERR_INTERNAL, "masked mirror group launch");
    else
        HIP_TRY(use8 ? launch_mirror8_group(g, b.d_c8, b.d_c8_meta, nq, e->metric, (int)e->grid_blocks.load(), st)
                     : launch_mirror_group(g, nq, e->metric, (int)e->grid_blocks.load(), st), WAX_HIP_ERR_INTERNAL, "mirror group launch");
    for (int i = 0; i < nq; ++i) {
        HIP_TRY(hipEventRecord(grp[i]->ev_done, st), WAX_HIP_ERR_INTERNAL, "event record");
        grp[i]->mirror = true;
        grp[i]->mirror8 = use8;
    }
    *took = true;
    e->st_mirror_scans += (uint64_t)nq;
    e->st_mirror_passes++;
    if (nq >= 2) { e->st_mirror_shared_passes++; e->st_mirror_shared_queries += (uint64_t)nq; }
    if (use8) e->st_mirror8_passes++;
    e->st_searches += (uint64_t)nq;
    // what the pass reads: every tile, unless every member reads the same bitmap and its count of live tiles has reached the host
    // (from the second pass on that entry on); members with different bitmaps are charged every tile — an upper bound
    uint64_t rows_read = e->count, live_tiles = 0, passing = 0;
    if (n_masked != 0) {
        e->pt_masked_passes++;
        e->pt_rode += (uint64_t)n_masked;
        if (one && pred_entry_counts(e, one_entry, false, &passing, &live_tiles)) rows_read = live_tiles * 16ull;
    }
    e->st_rows += rows_read * (uint64_t)nq;
    e->st_bytes += rows_read * (use8 ? (uint64_t)e->dims + 8ull : (uint64_t)e->dims * 2ull) + (uint64_t)nq * MIRROR_KP * e->dims * 4ull;
    return WAX_HIP_OK;
}

// Launch whatever is parked (share_mu held). A launch that fails is reported by the collect of every ticket it carried.
static void launch_parked(wax_hip_engine* e) {
    std::vector<Slot*> grp;
    grp.swap(e->parked);
    e->n_parked.store(0);
    if (grp.empty()) return;
    // A set with a predicate ticket in it takes the masked pass over the code mirror. Where that mirror cannot be had — an unmasked
    // member does not want it, or it cannot be prepared — the masked members leave the set for the blocking body and the rest goes on
    // as ever.
    bool masked = false, all8 = true;
    for (Slot* s : grp) { masked = masked || s->has_pred; all8 = all8 && s->want8; }
    int use8_hint = -1;
    if (masked) {
        use8_hint = all8 && mirror8_ready(e, grp[0]->stream, (uint64_t)grp.size()) ? 1 : 0;
        if (use8_hint == 0) {
            std::vector<Slot*> rest;
            for (Slot* s : grp) { if (s->has_pred) pred_ticket_defer(e, s); else rest.push_back(s); }
            grp.swap(rest);
            masked = false;
            if (grp.empty()) return;
            if (all8) use8_hint = 0; else use8_hint = -1;   // (not prepared: bf16 without asking again; else the set decides as ever)
        }
    }
    const int nq = (int)grp.size();
    const bool lone = nq == 1 && !masked;
    bool took = false;
    int rc;
    if (lone) rc = enqueue_mirror_scan(e, grp[0], grp[0]->h_query, grp[0]->q_norm, grp[0]->k_eff, 0, &took, grp[0]->want8 && use8_hint != 0);   // alone after all: the lone query's kernels
    else rc = enqueue_mirror_group(e, grp.data(), nq, &took, use8_hint);
    if (rc == WAX_HIP_OK && took) {
        if (lone) {
            const hipError_t err = hipEventRecord(grp[0]->ev_done, grp[0]->stream);
            if (err != hipSuccess) rc = fail(WAX_HIP_ERR_INTERNAL, std::string("event record: ") + hipGetErrorString(err));
        }
        if (rc == WAX_HIP_OK) {
            e->share_last = grp[0]->ev_done;
            for (Slot* s : grp) { s->listed = true; e->share_launched.push_back(s); }
        }
    } else if (rc == WAX_HIP_OK) {
        for (Slot* s : grp) {             // no mirror: every member takes the f32 scan on its own stream
            const int frc = parked_take_f32(e, s);
            if (frc != WAX_HIP_OK) { s->park_rc = frc; s->park_err = g_last_error; }
        }
    }
    if (rc != WAX_HIP_OK) {
        const std::string keep = g_last_error;
        (void)hipStreamSynchronize(grp[0]->stream);   // nothing of a half-enqueued group still runs when its tickets report the error
        (void)hipGetLastError();
        g_last_error = keep;
        for (Slot* s : grp) { s->park_rc = rc; s->park_err = keep; }
    }
}

// is a mirror pass of this engine still running? (share_mu held)
static bool mirror_pass_in_flight(wax_hip_engine* e) {
    return e->share_last != nullptr && hipEventQuery(e->share_last) == hipErrorNotReady;
}
