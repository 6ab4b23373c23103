// api_search.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: search_submit / search_collect / search, result capacity; the routing of predicate tickets (wax_hip_search_predicate_submit, filter_host.inc)

// ---- search ---------------------------------------------------------------

// try_only: never block waiting for a scratch slot (returns kSlotBusy) — used by callers that already hold
// tickets, which must collect one instead of waiting (two such callers would starve each other).
// caller_locked: the caller already holds the engine's shared lock and has flushed pending rows (wax_hip_search_many runs one
// snapshot over many engines): the ticket then owns no lock — it is collected with caller_locked too, inside the same scope.
// x: what wax_hip_search_predicate_submit adds to the ticket (TicketExtras, engine_types.inc)
static int submit_impl(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, uint64_t* out_ticket,
                       bool try_only, bool caller_locked = false, const TicketExtras* x = nullptr);

int wax_hip_search_submit(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, uint64_t* out_ticket) {
    if (e && e->sh) return sh_submit(e, query, dims, top_k, out_ticket);
    return submit_impl(e, query, dims, top_k, out_ticket, false);
}

// filter_host.inc
static inline bool predicate_passes(const wax_hip_row_predicate& p, int64_t ts, uint32_t fl);
static bool predicate_uses_mirror(wax_hip_engine* e, int kpad);
struct TermReq;   // api_terms.inc: the distinct required terms of a term search (null: none)
static int search_rows_locked(wax_hip_engine* e, const float* query, uint32_t dims, int kpad, int has_allow, const uint64_t* allow_frame_ids,
                              uint64_t n_allow, const wax_hip_row_predicate* pred, uint64_t* out_ids, float* out_scores,
                              uint32_t out_capacity, uint32_t* out_n, const TermReq* req = nullptr);
static inline void apply_min_score(float cut, uint64_t* ids, float* scores, uint32_t* n);

// what every ticket starts from
static void reset_ticket_extras(Slot* s, const TicketExtras* x, int32_t top_k) {
    s->has_cut = x != nullptr && x->has_cut != 0;
    s->cut = x != nullptr ? x->cut : 0.f;
    s->has_pred = false;
    s->pred_deferred = false;
    s->pred_entry = -1;
    s->top_k = top_k;
}

static int submit_impl(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, uint64_t* out_ticket,
                       bool try_only, bool caller_locked, const TicketExtras* x) {
    if (!e || !out_ticket) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine/ticket is null");
    DeviceGuard g(e->device);
    if (!caller_locked) {
        e->lock.lock_shared(holding(e) > 0);             // withReadLock (:447)
        { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) { e->lock.unlock_shared(); return frc; } }   // staged single-frame appends reach HBM here
    }
    const bool others_in_flight = !e->tickets.empty();   // uncollected single-query tickets of this engine, whoever holds them
    Slot* s = nullptr;
    int rc = WAX_HIP_OK;
    do {
        if (e->count == 0) {                               // :448 — an empty ticket, no GPU work
            rc = take_slot(e, &s, try_only, holding(e) > 0);
            if (rc != WAX_HIP_OK) break;
            s->k_eff = 0; s->timed = false; s->shared = false; s->listed = false;
            reset_ticket_extras(s, x, top_k);
            break;
        }
        if (dims != e->dims || !query) {                   // validate (:449, 830-833)
            rc = fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, query ? dims : 0));
            break;
        }
        if (e->row_base + e->count > 0x100000000ull) {
            rc = fail(WAX_HIP_ERR_CAPACITY, "row_base + count exceeds UInt32 row indices");
            break;
        }
        const int limit = clamp_topk(top_k);               // :450
        const int k_eff = (uint64_t)limit < e->count ? limit : (int)e->count;  // :451
        rc = take_slot(e, &s, try_only, holding(e) > 0);
        if (rc != WAX_HIP_OK) break;
        s->k_eff = k_eff;
        const int tk_mode = (int)e->time_kernels.load();   // read once per submit
        s->timed = tk_mode != 0;
        const float qn = query_norm(query, dims);
        hipError_t err = hipSuccess;
        s->mirror = false;
        s->mirror8 = false;
        s->want8 = false;
        s->flag_wait = false;
        bool mirrored = false;
        s->shared = false;
        s->listed = false;
        s->park_rc = WAX_HIP_OK;
        reset_ticket_extras(s, x, top_k);
        // ---- a ticket with a row predicate: decided on the host, riding a masked pass over the code mirror, or deferred ----
        bool ride = false;
        if (x != nullptr && x->pred != nullptr) {
            e->pt_submitted++;
            if (!e->cols.has_attributes()) {
                // a store on which attributes were never set reads (0, 0) in every row: every row passes or none does
                e->pt_host_decided++;
                if (!predicate_passes(*x->pred, 0, 0u)) { s->k_eff = 0; s->timed = false; break; }   // count 0, no device work
            } else {
                s->has_pred = true;
                s->pred = *x->pred;
                std::memcpy(s->h_query, query, (size_t)dims * sizeof(float));     // the blocking body's, should it answer at collect
                s->q_norm = qn;
                ride = e->force_general.load() == 0 && predicate_uses_mirror(e, k_eff) && mirror8_take(e, k_eff);
                if (ride) {
                    s->pred_entry = pred_entry_acquire(e, s->pred);
                    uint64_t passing = 0, tiles = 0;
                    ride = s->pred_entry >= 0 && !(pred_entry_counts(e, s->pred_entry, false, &passing, &tiles) && passing <= (uint64_t)MIRROR_KP);
                }
                if (!ride) { pred_ticket_defer(e, s); break; }
            }
        }
        if (ride || (!s->has_pred && scan_uses_mirror(e, k_eff))) {
            s->want8 = ride ? true : mirror8_take(e, k_eff);
            const int64_t share = mirror_share_mode(e, tk_mode);
            std::unique_lock<std::mutex> sg(e->share_mu, std::defer_lock);
            if (share != 0) {
                // "mirror_share": a query that arrives while a pass over the mirror is running waits for company — it is parked (its
                // query in the slot's pinned h_query) and launched with whatever else is parked by then: when the set is full, by the
                // collect of a parked ticket, or by a submit that finds the GPU without a pass. A lone query launches at once, as ever.
                // "mirror_fill" 1 (mode 1): mirror tickets that are launched and not yet collected are either finished — their caller is
                // draining a pass and its next submits are on the way — or a pass in flight; behind either a submit is parked, and it
                // launches the set only when it fills it. (share_last alone is one event of the last pass: right after the collect of a
                // group's first member its other members' events may not have signalled yet.) 0: the eager rule.
                sg.lock();
                const bool fill = share == 1 && e->mirror_fill.load() != 0;
                const bool waiting = fill && !e->share_launched.empty();
                if (share >= 2 || !e->parked.empty() || waiting || mirror_pass_in_flight(e)) {
                    std::memcpy(s->h_query, query, (size_t)dims * sizeof(float));
                    s->q_norm = qn;
                    s->mirror = true;
                    s->shared = true;
                    e->parked.push_back(s);
                    e->n_parked.store((int)e->parked.size());
                    if ((int)e->parked.size() >= MIRROR_MAX_NQ) launch_parked(e);
                    else if (share < 2 && !mirror_pass_in_flight(e)) {
                        if (waiting) e->st_mirror_fill_holds++;      // the eager rule would have launched here
                        else launch_parked(e);
                    }
                    break;
                }
            }
            if (ride) {
                // alone and at once: the masked pass of one member (its query is in h_query already)
                if (!mirror8_ready(e, s->stream, 1)) { pred_ticket_defer(e, s); break; }
                Slot* one[1] = {s};
                rc = enqueue_mirror_group(e, one, 1, &mirrored, 1);
            } else {
                rc = enqueue_mirror_scan(e, s, query, qn, k_eff, tk_mode, &mirrored, s->want8);
            }
            if (rc != WAX_HIP_OK) break;
            if (mirrored && share != 0) e->share_last = s->ev_done;   // (recorded just below, still under share_mu)
            if (mirrored) {
                err = ride ? hipSuccess : hipEventRecord(s->ev_done, s->stream);   // (the group launch has recorded its members')
                if (err != hipSuccess) { rc = fail(WAX_HIP_ERR_INTERNAL, std::string("event record: ") + hipGetErrorString(err)); break; }
                if (share != 0) { s->listed = true; e->share_launched.push_back(s); }
                break;
            }
        }
        const bool overlap = scan_overlaps_merge(e, others_in_flight);
        const bool qargs = scan_uses_query_args(e, k_eff, true, overlap);
        if (!qargs) {
            std::memcpy(s->h_query, query, (size_t)dims * sizeof(float));  // :467-468
            err = hipMemcpyAsync(s->d_query, s->h_query, (size_t)dims * sizeof(float), hipMemcpyHostToDevice, s->stream);
            if (err != hipSuccess) { rc = fail(WAX_HIP_ERR_INTERNAL, std::string("query upload: ") + hipGetErrorString(err)); break; }
        } else {
            e->st_query_args++;      // the query rides in the launch packet: no copy on the stream
        }
        // The last kernel of the chain writes the k hits straight into the slot's pinned host buffer
        // (device-visible, 16*k bytes over PCIe): no D2H copy launch; visibility at ev_done.
        // "done_flag" (default 1): a scan that merges in the kernel (small grids) publishes a completion word in pinned memory behind
        // its hits and collect polls that word — no event behind the kernel. Not while kernels are timed (the timing events must have
        // completed when collect reads them).
        const bool want_flag = e->done_flag.load() != 0 && !s->timed && s->coherent;
        s->flag_wait = false;
        if (want_flag) s->done_seq += 1;
        bool flagged = false;
        rc = enqueue_scan(e, qargs ? nullptr : s->d_query, qn, k_eff, k_eff, s->d_partials, s, s->h_hits, s->stream,
                          s->timed ? s->ev0 : nullptr, s->timed ? s->ev1 : nullptr, /*chain=*/chain_scans(e, tk_mode), &s->t_start, &s->t_end, query,
                          want_flag ? s->h_done : nullptr, s->done_seq, &flagged, overlap, tk_mode);
        if (rc != WAX_HIP_OK) break;
        if (flagged) {
            s->flag_wait = true;
            e->st_flag_waits++;
        } else {
            err = hipEventRecord(s->ev_done, s->stream);
            if (err != hipSuccess) { rc = fail(WAX_HIP_ERR_INTERNAL, std::string("event record: ") + hipGetErrorString(err)); break; }
        }
    } while (0);
    if (rc != WAX_HIP_OK) {
        if (s) { (void)hipStreamSynchronize(s->stream); pred_entry_release(e, s->pred_entry); s->pred_entry = -1; e->slots.release(s); }
        if (!caller_locked) e->lock.unlock_shared();
        return rc;
    }
    *out_ticket = e->tickets.put(s);
    e->holders.note_submit(&s->owner);
    return WAX_HIP_OK;  // shared lock stays held until collect (caller_locked: until the caller's scope ends)
}

// Shared tail of collect: either converts to (ids, scores) or hands back the raw hits (padded to kcap).
// `capacity`: entries the (ids, scores) arrays hold; `hits_cap`: entries of out_hits (every one is written).
static int collect_impl(wax_hip_engine* e, uint64_t ticket, uint64_t* out_ids, float* out_scores, uint32_t capacity,
                        uint32_t* out_count, wax_hip_hit* out_hits, uint32_t hits_cap, bool caller_locked = false);

int wax_hip_search_collect(wax_hip_engine* e, uint64_t ticket, uint64_t* out_ids, float* out_scores, uint32_t out_capacity,
                           uint32_t* out_count) {
    if (e && e->sh) return sh_collect(e, ticket, out_ids, out_scores, out_capacity, out_count);
    return collect_impl(e, ticket, out_ids, out_scores, out_capacity, out_count, nullptr, 0);
}

static int collect_impl(wax_hip_engine* e, uint64_t ticket, uint64_t* out_ids, float* out_scores, uint32_t capacity,
                        uint32_t* out_count, wax_hip_hit* out_hits, uint32_t hits_cap, bool caller_locked) {
    if (!e || !out_count) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine/out_count is null");
    DeviceGuard g(e->device);
    Slot* s = nullptr;
    if (!e->tickets.take(ticket, &s)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "unknown ticket " + std::to_string(ticket));
    int rc = WAX_HIP_OK;
    *out_count = 0;
    if (s->k_eff == 0 && out_hits)
        for (uint32_t i = 0; i < hits_cap; ++i) out_hits[i] = wax_hip_hit{KEY_PAD, ID_PAD};
    if (s->k_eff > 0 && (s->shared || s->listed || e->n_parked.load() > 0)) {
        // "mirror_share": a parked ticket is launched now, with everything parked beside it. Under "mirror_fill" 0 any other collect
        // that is about to block launches what is parked first (queued behind the pass in flight, so the GPU never waits for the
        // host); under "mirror_fill" 1 it holds the set — its caller submits again as soon as it returns, and those submits fill it.
        // Mode 2 launches only for a ticket that is itself parked.
        std::unique_lock<std::mutex> sg(e->share_mu);
        const bool mine = std::find(e->parked.begin(), e->parked.end(), s) != e->parked.end();
        if (mine) launch_parked(e);
        else if (!e->parked.empty() && e->mirror_share.load() < 2) {
            const bool blocks = s->flag_wait ? __atomic_load_n(s->h_done, __ATOMIC_ACQUIRE) != s->done_seq
                                             : hipEventQuery(s->ev_done) == hipErrorNotReady;
            if (blocks) {
                if (e->mirror_fill.load() != 0) e->st_mirror_fill_holds++;
                else launch_parked(e);
            }
        }
        if (s->listed) {               // (launch_parked lists a parked ticket: looked at after it)
            auto it = std::find(e->share_launched.begin(), e->share_launched.end(), s);
            if (it != e->share_launched.end()) e->share_launched.erase(it);
            s->listed = false;
        }
        if (s->shared && s->park_rc != WAX_HIP_OK) rc = fail(s->park_rc, s->park_err);
    }
    // a predicate ticket that did not ride, or rode without a certificate: the blocking body, under the lock the ticket holds
    auto blocking_body = [&]() -> int {
        if ((!out_ids || !out_scores) && capacity > 0) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "output arrays are null");
        return search_rows_locked(e, s->h_query, e->dims, clamp_topk(s->top_k), 0, nullptr, 0, &s->pred, out_ids, out_scores, capacity, out_count);
    };
    bool deferred = false;
    if (s->has_pred) {
        if (s->shared) { std::unique_lock<std::mutex> sg(e->share_mu); deferred = s->pred_deferred; }   // (the set's launch may have written it)
        else deferred = s->pred_deferred;
        if (deferred && rc == WAX_HIP_OK) rc = out_hits ? fail(WAX_HIP_ERR_INTERNAL, "a predicate ticket has no raw-hit form") : blocking_body();
    }
    if (s->k_eff > 0 && rc == WAX_HIP_OK && !deferred) {
        hipError_t err = hipSuccess;
        if (s->flag_wait) {
            // poll the completion word the kernel's last workgroup publishes behind the hits (system-scope release). The stream is
            // queried now and then so that a kernel that died without publishing fails loudly instead of spinning for ever.
            // Spin for a bounded time (the scans this path serves take 10 - 300 us), then give the core away between polls: many
            // collecting threads behind a busy stream must not each burn a core.
            const uint64_t want = s->done_seq;
            const auto t_spin = std::chrono::steady_clock::now();
            bool polite = false;
            for (uint32_t spins = 1;; ++spins) {
                if (__atomic_load_n(s->h_done, __ATOMIC_ACQUIRE) == want) break;
                if (!polite) {
                    cpu_relax();
                    if ((spins & 0x3ffu) == 0u &&
                        std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_spin).count() > 400)
                        polite = true;
                } else {
                    std::this_thread::yield();
                    if ((spins & 0xffu) == 0u) std::this_thread::sleep_for(std::chrono::microseconds(50));
                }
                if ((spins & 0x3fffu) == 0u || (polite && (spins & 0x3fu) == 0u)) {
                    const hipError_t qs = hipStreamQuery(s->stream);
                    if (qs == hipErrorNotReady) continue;
                    if (__atomic_load_n(s->h_done, __ATOMIC_ACQUIRE) == want) break;
                    err = qs == hipSuccess ? hipErrorUnknown : qs;   // the stream drained (or failed) and the word never came
                    break;
                }
            }
        } else {
            err = hipEventSynchronize(s->ev_done);   // commandBuffer completion (:577-582); later queries on the stream keep running
        }
        bool certified = err == hipSuccess && s->mirror && __atomic_load_n(slot_cert_word(s->h_done), __ATOMIC_ACQUIRE) == 1u;
        bool tells = true;                 // the certificate says something about the corpus: it feeds the "mirror_bits" breaker
        if (err == hipSuccess && s->mirror && s->has_pred) {
            // a bitmap of MIRROR_KP or fewer passing rows never certifies (the blocking call does not take the mirror there either)
            uint64_t passing = 0, tiles = 0;
            if (!pred_entry_counts(e, s->pred_entry, true, &passing, &tiles) || passing <= (uint64_t)MIRROR_KP) { certified = false; tells = false; }
            if (certified) { e->pt_certified++; e->st_predicate_searches++; }
        }
        if (err == hipSuccess && s->mirror && s->mirror8 && tells) mirror8_note_result(e, certified);
        if (err == hipSuccess && s->mirror && !certified && s->has_pred) {
            e->pt_fallbacks++;
            e->st_mirror_fallbacks++;
            if (s->mirror8) e->st_mirror8_fallbacks++;
            rc = out_hits ? fail(WAX_HIP_ERR_INTERNAL, "a predicate ticket has no raw-hit form") : blocking_body();
            deferred = true;               // answered: nothing below converts hits
        } else if (err == hipSuccess && s->mirror && !certified) {
            // the mirror's certificate failed (ties, a clustered store, zero / NaN rows or query): this query is re-run on the f32 scan,
            // on the same slot, and that answer is returned (the batched path's "uncertified queries are re-run exactly at collect")
            e->st_mirror_fallbacks++;
            if (s->mirror8) e->st_mirror8_fallbacks++;
            rc = enqueue_scan(e, nullptr, s->q_norm, s->k_eff, s->k_eff, s->d_partials, s, s->h_hits, s->stream, nullptr, nullptr,
                              /*chain=*/false, nullptr, nullptr, s->h_query);
            if (rc != WAX_HIP_OK) err = hipErrorUnknown;
            else err = hipStreamSynchronize(s->stream);
        }
        if (err != hipSuccess) {
            rc = fail(WAX_HIP_ERR_INTERNAL, std::string("search failed on device: ") + hipGetErrorString(err));
            // a scan that died part-way leaves its fused-merge ticket half counted; no later scan on this slot could ever be
            // "last arriver" again and callers would read stale hits with no error. Re-arm it (best effort: after a device
            // fault the runtime usually refuses this too, and every later call on the slot then fails loudly as well).
            std::string keep = g_last_error;
            (void)hipStreamSynchronize(s->stream);
            (void)hipMemsetAsync(partials_ticket(s->d_partials), 0, 128, s->stream);
            (void)hipStreamSynchronize(s->stream);
            (void)hipGetLastError();
            g_last_error = keep;
        } else if (!deferred) {
            if (s->timed) {
                float ms = 0.f;
                if (s->t_start && s->t_end && hipEventElapsedTime(&ms, s->t_start, s->t_end) == hipSuccess) {
                    std::unique_lock<std::mutex> sg(e->st_mu);
                    e->st_last_ms = ms; e->st_total_ms += ms; e->st_timed += 1;
                }
            }
            if (out_hits) {
                uint32_t m = 0;
                for (uint32_t i = 0; i < hits_cap; ++i) {
                    out_hits[i] = (i < (uint32_t)s->k_eff) ? s->h_hits[i] : wax_hip_hit{KEY_PAD, ID_PAD};
                    if (out_hits[i].key != KEY_PAD) ++m;
                }
                *out_count = m;
            } else if ((!out_ids || !out_scores) && capacity > 0) {
                rc = fail(WAX_HIP_ERR_INVALID_ARGUMENT, "output arrays are null");
            } else {
                rc = hits_to_results(e->metric, s->h_hits, (uint32_t)s->k_eff, out_ids, out_scores, capacity, out_count);
            }
        }
    }
    if (rc == WAX_HIP_OK && s->has_cut && !out_hits && out_ids && out_scores) apply_min_score(s->cut, out_ids, out_scores, out_count);
    pred_entry_release(e, s->pred_entry);
    s->pred_entry = -1;
    e->holders.note_collect(s->owner);
    e->slots.release(s);
    if (!caller_locked) e->lock.unlock_shared();   // (a ticket submitted with caller_locked never took it)
    return rc;
}

uint32_t wax_hip_result_capacity(int32_t top_k) { return (uint32_t)clamp_topk(top_k); }

int wax_hip_search(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, uint64_t* out_ids,
                   float* out_scores, uint32_t out_capacity, uint32_t* out_count) {
    uint64_t t = 0;
    int rc = wax_hip_search_submit(e, query, dims, top_k, &t);
    if (rc != WAX_HIP_OK) return rc;
    return wax_hip_search_collect(e, t, out_ids, out_scores, out_capacity, out_count);
}
