// tuning.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: stats, the tuning table and the set / get calls that look a key up in it (the one place a key or a counter is added), the two
// timing microbenchmarks, the code mirror's diagnostic read-outs

// ---- observability / tuning -----------------------------------------------

int wax_hip_stats(wax_hip_engine* e, wax_hip_stats_t* out) {
    if (!e || !out) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (e->sh) return sh_stats(e, out);
    out->searches = e->st_searches.load();
    out->rows_scanned = e->st_rows.load();
    out->bytes_scanned = e->st_bytes.load();
    out->transient_allocations = e->st_alloc.load();
    out->reuse_count = e->st_reuse.load();
    out->reserved_rows = e->capacity;
    {
        DeviceGuard g(e->device);
        for (int r = 0; r < kShardRing; ++r) harvest_ring_event(e, r);
    }
    std::unique_lock<std::mutex> sg(e->st_mu);
    out->last_scan_kernel_ms = e->st_last_ms;
    out->scan_kernel_ms_total = e->st_total_ms;
    out->scan_kernels_timed = e->st_timed;
    out->batch_gemm_ms_total = e->st_gemm_ms;
    out->batch_gemms_timed = e->st_gemm_timed;
    out->batch_gemm_rows = e->st_gemm_rows;
    out->batch_gemm_queries = e->st_gemm_queries;
    return WAX_HIP_OK;
}

}  // extern "C"

// ---- the tuning table -------------------------------------------------------
// One row per key of a single-device engine: how wax_hip_set_tuning checks and stores a value, what wax_hip_get_tuning loads, and
// what a sharded handle answers (sh_get_tuning). A key or a counter is added HERE and documented in include/wax_hip.h; nothing
// else names it. (The keys of the sharded handle itself, "exchange", "shard_min_mb", ..., are code in sharded.inc.)
namespace {

using Knob = std::atomic<int64_t> wax_hip_engine::*;
using Counter = std::atomic<uint64_t> wax_hip_engine::*;
struct TuningSet {
    enum Kind : uint8_t { NONE, ANY, FLAG, RANGE, ONE_OF, MASK, FN } kind;
    Knob knob;                              // ANY .. MASK: where the value goes (FLAG: as value != 0)
    int64_t a, b, c;                        // RANGE and FN: [a, b]. ONE_OF: a, b or c. MASK: the bits of a
    const char* refusal;                    // the message of a refused value
    int (*fn)(wax_hip_engine*, int64_t);    // FN: a side effect or a target that is no Knob; called with a value in [a, b], returns the status
};
struct TuningGet {                          // at most one is set; none: the key reads -1
    Knob knob;
    Counter counter;
    int64_t (*fn)(wax_hip_engine*);
};
enum TuningSharded : uint8_t { FIRST_SHARD, SUM_SHARDS };   // what a sharded handle answers: its first shard's value / the sum over its shards
struct TuningRow { const char* name; TuningSet set; TuningGet get; TuningSharded sharded; };

constexpr TuningSet not_set() { return {TuningSet::NONE, nullptr, 0, 0, 0, nullptr, nullptr}; }
constexpr TuningSet set_any(Knob k) { return {TuningSet::ANY, k, 0, 0, 0, nullptr, nullptr}; }
constexpr TuningSet set_flag(Knob k) { return {TuningSet::FLAG, k, 0, 0, 0, nullptr, nullptr}; }
constexpr TuningSet set_range(Knob k, int64_t lo, int64_t hi, const char* refusal) { return {TuningSet::RANGE, k, lo, hi, 0, refusal, nullptr}; }
constexpr TuningSet set_one_of(Knob k, int64_t a, int64_t b, int64_t c, const char* refusal) { return {TuningSet::ONE_OF, k, a, b, c, refusal, nullptr}; }
constexpr TuningSet set_mask(Knob k, int64_t bits, const char* refusal) { return {TuningSet::MASK, k, bits, 0, 0, refusal, nullptr}; }
constexpr TuningSet set_fn(int (*fn)(wax_hip_engine*, int64_t), int64_t lo, int64_t hi, const char* refusal) { return {TuningSet::FN, nullptr, lo, hi, 0, refusal, fn}; }
constexpr TuningGet not_get() { return {nullptr, nullptr, nullptr}; }
constexpr TuningGet get_knob(Knob k) { return {k, nullptr, nullptr}; }
constexpr TuningGet get_counter(Counter c) { return {nullptr, c, nullptr}; }
constexpr TuningGet get_fn(int64_t (*fn)(wax_hip_engine*)) { return {nullptr, nullptr, fn}; }
#define GET_EXPR(expr) get_fn([](wax_hip_engine* e) -> int64_t { return (int64_t)(expr); })

// the FN setters (the row's range, where it has one, is checked before they are called)
int set_batch_workspaces(wax_hip_engine* e, int64_t v) { e->bctxs.set_cap((int)v); return WAX_HIP_OK; }
int set_streams(wax_hip_engine* e, int64_t v) { e->n_streams = (int)v; return WAX_HIP_OK; }
int set_slots(wax_hip_engine* e, int64_t v) { e->slots.set_cap((int)v); return WAX_HIP_OK; }
int set_retry_hint(wax_hip_engine* e, int64_t v) { e->retry_hint = (int)v; return WAX_HIP_OK; }   // > 0: the next `v` clean batches still carry the device-side retry kernel (set by collect; tests force it)
int set_merge_overlap_mb(wax_hip_engine* e, int64_t v) { e->merge_overlap_mb = v < 0 ? 0 : v; return WAX_HIP_OK; }
int set_batch_first(wax_hip_engine* e, int64_t v) {
    if (v < 128 || v > kBatchFirstSlab || v % 128) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "batch_first must be a multiple of 128 in 128..2048");
    e->batch_first = v;
    return WAX_HIP_OK;
}
int set_reset_stats(wax_hip_engine* e, int64_t) {
    e->st_searches = 0; e->st_rows = 0; e->st_bytes = 0;
    {
        DeviceGuard g(e->device);
        for (int r = 0; r < kShardRing; ++r) harvest_ring_event(e, r);
    }
    std::unique_lock<std::mutex> sg(e->st_mu);
    e->st_last_ms = 0; e->st_total_ms = 0; e->st_timed = 0;
    e->st_gemm_ms = 0; e->st_gemm_timed = 0; e->st_gemm_rows = 0; e->st_gemm_queries = 0;
    return WAX_HIP_OK;
}
// the getters that read device words (blocking)
int64_t get_short_select_failures(wax_hip_engine* e) {   // short selections whose certificate failed (the long path answered): every slot's
    int64_t t = 0;
    DeviceGuard g(e->device);
    (void)hipDeviceSynchronize();
    e->slots.for_each([&t](Slot* sl) {
        uint32_t f[4] = {0u, 0u, 0u, 0u};
        if (sl->sw_ready && sl->sw.flags && hipMemcpy(f, sl->sw.flags, sizeof(f), hipMemcpyDeviceToHost) == hipSuccess) t += f[1];
        if (sl->d_partials && hipMemcpy(f, partials_ticket(sl->d_partials) + 8, sizeof(f), hipMemcpyDeviceToHost) == hipSuccess) t += f[1];   // the fused path's short merge
    });
    for (int r = 0; r < kShardRing; ++r) {
        uint32_t f[4] = {0u, 0u, 0u, 0u};
        if (e->ring_d_partials[r] && hipMemcpy(f, partials_ticket(e->ring_d_partials[r]) + 8, sizeof(f), hipMemcpyDeviceToHost) == hipSuccess) t += f[1];
    }
    return t;
}
double mirror_measured_bound(wax_hip_engine* e, int which) {   // the mirror's measured bounds: 0 = the largest norm, 1 = the largest row error
    unsigned int bits[2] = {0u, 0u};
    if (e->batch.d_maxnorm) {
        DeviceGuard g(e->device);
        (void)hipDeviceSynchronize();
        (void)hipMemcpy(bits, e->batch.d_maxnorm, sizeof(bits), hipMemcpyDeviceToHost);
    }
    float f[2];
    std::memcpy(f, bits, sizeof(f));
    return (double)f[which];
}

constexpr TuningRow kTuning[] = {
    {"grid_blocks", set_any(&wax_hip_engine::grid_blocks), get_knob(&wax_hip_engine::grid_blocks), FIRST_SHARD},
    {"variant", set_any(&wax_hip_engine::variant), get_knob(&wax_hip_engine::variant), FIRST_SHARD},
    {"variant_count", not_set(), GET_EXPR(scan_variant_count(e->dims)), FIRST_SHARD},
    {"scan_grid", not_set(), GET_EXPR(scan_grid_for((uint32_t)e->count, e->dims, (int)e->variant.load(), (int)e->grid_blocks.load())), FIRST_SHARD},
    {"fused_max_k", not_set(), GET_EXPR(FUSED_MAX_K), FIRST_SHARD},
    {"time_kernels", set_any(&wax_hip_engine::time_kernels), get_knob(&wax_hip_engine::time_kernels), FIRST_SHARD},
    {"force_general", set_any(&wax_hip_engine::force_general), get_knob(&wax_hip_engine::force_general), FIRST_SHARD},
    {"select_grid", set_range(&wax_hip_engine::select_grid, 0, 2048, "select_grid must be 0 (auto) .. 2048"), get_knob(&wax_hip_engine::select_grid), FIRST_SHARD},
    {"select_short", set_range(&wax_hip_engine::select_short, 0, 2, "select_short must be 0, 1 or 2"), get_knob(&wax_hip_engine::select_short), FIRST_SHARD},
    {"short_selects", not_set(), get_counter(&wax_hip_engine::st_short_selects), SUM_SHARDS},
    {"short_select_failures", not_set(), get_fn(get_short_select_failures), SUM_SHARDS},
    {"stream_nt", set_any(&wax_hip_engine::stream_nt), get_knob(&wax_hip_engine::stream_nt), FIRST_SHARD},
    {"fuse_merge", set_flag(&wax_hip_engine::fuse_merge), get_knob(&wax_hip_engine::fuse_merge), FIRST_SHARD},
    {"merged_scans", not_set(), get_counter(&wax_hip_engine::st_merged_scans), FIRST_SHARD},   // a counter, yet not summed: as found, to be decided
    {"done_flag", set_flag(&wax_hip_engine::done_flag), get_knob(&wax_hip_engine::done_flag), FIRST_SHARD},
    {"done_flag_waits", not_set(), get_counter(&wax_hip_engine::st_flag_waits), FIRST_SHARD},   // a counter, yet not summed: as found, to be decided
    {"merge_kway", set_flag(&wax_hip_engine::merge_kway), get_knob(&wax_hip_engine::merge_kway), FIRST_SHARD},
    {"merge_overlap_mb", set_fn(set_merge_overlap_mb, INT64_MIN, INT64_MAX, nullptr), get_knob(&wax_hip_engine::merge_overlap_mb), FIRST_SHARD},
    {"overlap_scans", not_set(), get_counter(&wax_hip_engine::st_overlap_scans), FIRST_SHARD},   // a counter, yet not summed: as found, to be decided
    {"query_args", set_range(&wax_hip_engine::query_args, 0, 2, "query_args must be 0, 1 or 2"), get_knob(&wax_hip_engine::query_args), FIRST_SHARD},
    {"query_args_scans", not_set(), get_counter(&wax_hip_engine::st_query_args), SUM_SHARDS},
    {"scan_plain_mb", set_any(&wax_hip_engine::scan_plain_mb), get_knob(&wax_hip_engine::scan_plain_mb), FIRST_SHARD},
    {"scan_chain", set_range(&wax_hip_engine::scan_chain, -1, 1, "scan_chain must be -1 (auto), 0 or 1"), get_knob(&wax_hip_engine::scan_chain), FIRST_SHARD},
    {"share_timing", set_flag(&wax_hip_engine::share_timing), get_knob(&wax_hip_engine::share_timing), FIRST_SHARD},   // 0: every chained scan records its own start event (one more packet between scans)
    {"streams", set_fn(set_streams, 1, kMaxStreams, "streams must be 1..4"), GET_EXPR(e->n_streams), FIRST_SHARD},
    {"slots", set_fn(set_slots, 1, 64, "slots must be 1..64"), GET_EXPR(e->slots.cap()), FIRST_SHARD},
    {"store_ptr", not_set(), GET_EXPR((uintptr_t)e->d_store), FIRST_SHARD},   // diagnosis: where the slab sits (tools/bimodal_probe.py)
    {"reset_stats", set_fn(set_reset_stats, INT64_MIN, INT64_MAX, nullptr), not_get(), FIRST_SHARD},
    {"scan_mirror", set_range(&wax_hip_engine::scan_mirror, 0, 2, "scan_mirror must be 0, 1 or 2"), get_knob(&wax_hip_engine::scan_mirror), FIRST_SHARD},
    {"mirror_scans", not_set(), get_counter(&wax_hip_engine::st_mirror_scans), SUM_SHARDS},
    {"mirror_scan_fallbacks", not_set(), get_counter(&wax_hip_engine::st_mirror_fallbacks), SUM_SHARDS},
    {"mirror_scan_unavailable", not_set(), get_counter(&wax_hip_engine::st_mirror_unavailable), SUM_SHARDS},
    {"mirror_share", set_range(&wax_hip_engine::mirror_share, 0, 2, "mirror_share must be 0, 1 or 2"), get_knob(&wax_hip_engine::mirror_share), FIRST_SHARD},
    {"mirror_passes", not_set(), get_counter(&wax_hip_engine::st_mirror_passes), SUM_SHARDS},   // scan launches over the mirror, whatever they carried
    {"mirror_shared_passes", not_set(), get_counter(&wax_hip_engine::st_mirror_shared_passes), SUM_SHARDS},   // ... of which with two or more queries
    {"mirror_shared_queries", not_set(), get_counter(&wax_hip_engine::st_mirror_shared_queries), SUM_SHARDS},   // queries answered by those
    {"mirror_fill", set_range(&wax_hip_engine::mirror_fill, 0, 1, "mirror_fill must be 0 or 1"), get_knob(&wax_hip_engine::mirror_fill), FIRST_SHARD},
    {"mirror_fill_holds", not_set(), get_counter(&wax_hip_engine::st_mirror_fill_holds), SUM_SHARDS},   // submits parked / held and blocking collects that held the parked set back ("mirror_fill" 1)
    {"mirror_bits", set_one_of(&wax_hip_engine::mirror_bits, 0, 8, 16, "mirror_bits must be 0, 8 or 16"), get_knob(&wax_hip_engine::mirror_bits), FIRST_SHARD},
    {"mirror8_passes", not_set(), get_counter(&wax_hip_engine::st_mirror8_passes), SUM_SHARDS},   // passes over the 8-bit code mirror (lone or shared; also counted in "mirror_passes")
    {"mirror8_fallbacks", not_set(), get_counter(&wax_hip_engine::st_mirror8_fallbacks), SUM_SHARDS},   // 8-bit queries whose certificate failed (also counted in "mirror_scan_fallbacks")
    {"mirror8_unavailable", not_set(), get_counter(&wax_hip_engine::st_mirror8_unavailable), SUM_SHARDS},   // queries sent to bf16 because the code mirror could not be prepared
    {"mirror8_breaker_trips", not_set(), get_counter(&wax_hip_engine::st_mirror8_breaker_trips), SUM_SHARDS},
    {"mirror8_conversions", not_set(), GET_EXPR(e->batch.conversions8.load()), SUM_SHARDS},   // code mirror: conversions enqueued / rows converted so far
    {"mirror8_rows_converted", not_set(), GET_EXPR(e->batch.rows8_converted.load()), SUM_SHARDS},
    {"mirror_conversions", not_set(), GET_EXPR(e->batch.conversions.load()), FIRST_SHARD},        // bf16 mirror: conversions enqueued / rows converted so far. A counter, yet not summed (its 8-bit twin is): as found, to be decided
    {"mirror_rows_converted", not_set(), GET_EXPR(e->batch.rows_converted.load()), FIRST_SHARD},  // a counter, yet not summed (its 8-bit twin is): as found, to be decided
    {"batch_min", set_any(&wax_hip_engine::batch_min), get_knob(&wax_hip_engine::batch_min), FIRST_SHARD},
    {"batch_mode", set_any(&wax_hip_engine::batch_mode), get_knob(&wax_hip_engine::batch_mode), FIRST_SHARD},
    {"batch_max_k", not_set(), GET_EXPR(kBatchMaxK), FIRST_SHARD},
    {"batch_queries", not_set(), get_counter(&wax_hip_engine::st_batch_queries), SUM_SHARDS},
    {"batch_fallbacks", not_set(), get_counter(&wax_hip_engine::st_batch_fallbacks), SUM_SHARDS},
    {"batch_qfrag", set_flag(&wax_hip_engine::batch_qfrag), get_knob(&wax_hip_engine::batch_qfrag), FIRST_SHARD},
    {"batch_rega", set_one_of(&wax_hip_engine::batch_rega, 0, 1, 5, "batch_rega must be 0, 1 or 5"), get_knob(&wax_hip_engine::batch_rega), FIRST_SHARD},
    {"batch_dyn_tail", set_range(&wax_hip_engine::batch_dyn_tail, 0, 1, "batch_dyn_tail must be 0 or 1"), get_knob(&wax_hip_engine::batch_dyn_tail), FIRST_SHARD},
    {"batch_host_multi", set_range(&wax_hip_engine::batch_host_multi, 0, 1, "batch_host_multi must be 0 or 1"), get_knob(&wax_hip_engine::batch_host_multi), FIRST_SHARD},
    {"batch_in_wait", set_range(&wax_hip_engine::batch_in_wait, 0, 1, "batch_in_wait must be 0 or 1"), get_knob(&wax_hip_engine::batch_in_wait), FIRST_SHARD},
    {"batch_debug", set_mask(&wax_hip_engine::batch_debug, 4096 | 16384 | 65536, "batch_debug: bits 4096, 16384, 65536 only"), not_get(), FIRST_SHARD},
    {"batch_prof_ptr", set_any(&wax_hip_engine::batch_prof_ptr), not_get(), FIRST_SHARD},
    {"batch_workspaces", set_fn(set_batch_workspaces, 1, 16, "batch_workspaces must be 1..16"), GET_EXPR(e->bctxs.cap()), FIRST_SHARD},
    {"batch_first", set_fn(set_batch_first, INT64_MIN, INT64_MAX, nullptr), get_knob(&wax_hip_engine::batch_first), FIRST_SHARD},
    {"batch_growth", set_range(&wax_hip_engine::batch_growth, 1, 64, "batch_growth must be 1..64"), get_knob(&wax_hip_engine::batch_growth), FIRST_SHARD},
    {"batch_slab_mb", set_range(&wax_hip_engine::batch_slab_mb, 1, 4096, "batch_slab_mb must be 1..4096"), get_knob(&wax_hip_engine::batch_slab_mb), FIRST_SHARD},
    {"batch_onepass", set_any(&wax_hip_engine::batch_onepass), get_knob(&wax_hip_engine::batch_onepass), FIRST_SHARD},
    {"batch_onepass_tiles", set_range(&wax_hip_engine::batch_onepass_tiles, 32, INT64_MAX, "batch_onepass_tiles must be >= 32"), get_knob(&wax_hip_engine::batch_onepass_tiles), FIRST_SHARD},
    {"onepass_queries", not_set(), get_counter(&wax_hip_engine::st_onepass_queries), SUM_SHARDS},
    {"batch_kp_fused", set_flag(&wax_hip_engine::batch_kp_fused), get_knob(&wax_hip_engine::batch_kp_fused), FIRST_SHARD},
    {"batch_survivors", set_range(&wax_hip_engine::batch_survivors, 2, 64, "batch_survivors must be 2..64"), get_knob(&wax_hip_engine::batch_survivors), FIRST_SHARD},
    {"batch_sample_div", set_range(&wax_hip_engine::batch_sample_div, 4, 4096, "batch_sample_div must be 4..4096"), get_knob(&wax_hip_engine::batch_sample_div), FIRST_SHARD},
    {"batch_eps_measured", set_flag(&wax_hip_engine::batch_eps_measured), get_knob(&wax_hip_engine::batch_eps_measured), FIRST_SHARD},
    {"batch_max_norm_e6", not_set(), GET_EXPR(mirror_measured_bound(e, 0) * 1e6), FIRST_SHARD},
    {"batch_max_row_err_e9", not_set(), GET_EXPR(mirror_measured_bound(e, 1) * 1e9), FIRST_SHARD},
    {"retry_hint", set_fn(set_retry_hint, 0, 1024, "retry_hint must be 0..1024"), GET_EXPR(e->retry_hint.load()), FIRST_SHARD},
    {"batch_retry", set_range(&wax_hip_engine::batch_retry, 0, 2, "batch_retry must be 0, 1 or 2"), get_knob(&wax_hip_engine::batch_retry), FIRST_SHARD},
    {"batch_retries", not_set(), get_counter(&wax_hip_engine::st_batch_retries), SUM_SHARDS},
    {"batch_inline_retries", not_set(), get_counter(&wax_hip_engine::st_batch_inline_retries), SUM_SHARDS},
    {"batch_multi", set_flag(&wax_hip_engine::batch_multi), get_knob(&wax_hip_engine::batch_multi), FIRST_SHARD},
    {"batch_multi_passes", not_set(), get_counter(&wax_hip_engine::st_multi_passes), SUM_SHARDS},
    {"batch_multi_queries", not_set(), get_counter(&wax_hip_engine::st_multi_queries), SUM_SHARDS},
    {"batch_multi_group", not_set(), GET_EXPR(scan_multi_group(e->dims, 10)), FIRST_SHARD},        // queries per shared exact pass, k <= 60 (64-slot lists)
    {"batch_multi_group_big", not_set(), GET_EXPR(scan_multi_group(e->dims, 192)), FIRST_SHARD},   // ... k <= 192 (256-slot lists)
    {"idhash_rows_inserted", not_set(), get_counter(&wax_hip_engine::st_idhash_rows), FIRST_SHARD},   // a counter, yet not summed: as found, to be decided
    {"filter_device_min", set_range(&wax_hip_engine::filter_device_min, -1, INT64_MAX, "filter_device_min must be >= -1"), get_knob(&wax_hip_engine::filter_device_min), FIRST_SHARD},
    {"filter_device_searches", not_set(), get_counter(&wax_hip_engine::st_filter_device), SUM_SHARDS},
    {"filter_batch", set_range(&wax_hip_engine::filter_batch, 0, 1, "filter_batch must be 0 or 1"), get_knob(&wax_hip_engine::filter_batch), FIRST_SHARD},
    {"filter_batch_queries", not_set(), get_counter(&wax_hip_engine::st_filter_batch_queries), SUM_SHARDS},
    {"filter_batch_fallbacks", not_set(), get_counter(&wax_hip_engine::st_filter_batch_fallbacks), SUM_SHARDS},
    {"predicate_route", set_range(&wax_hip_engine::predicate_route, 0, 2, "predicate_route must be 0 (auto), 1 (gather) or 2 (masked scan)"), get_knob(&wax_hip_engine::predicate_route), FIRST_SHARD},
    {"predicate_scan_min_permille", set_range(&wax_hip_engine::predicate_scan_min_permille, 0, 1001, "predicate_scan_min_permille must be 0..1001"), get_knob(&wax_hip_engine::predicate_scan_min_permille), FIRST_SHARD},
    {"predicate_searches", not_set(), get_counter(&wax_hip_engine::st_predicate_searches), SUM_SHARDS},   // wax_hip_search_predicate calls with a non-empty predicate
    {"predicate_gather_searches", not_set(), get_counter(&wax_hip_engine::st_predicate_gather), SUM_SHARDS},   // ... answered by gathering the passing rows
    {"predicate_masked_scans", not_set(), get_counter(&wax_hip_engine::st_predicate_masked), SUM_SHARDS},   // ... answered by the masked f32 scan
    {"predicate_chunks_skipped", not_set(), get_counter(&wax_hip_engine::st_predicate_skipped), SUM_SHARDS},   // chunks those scans did not load
    {"predicate_mirror", set_range(&wax_hip_engine::predicate_mirror, 0, 2, "predicate_mirror must be 0 (never), 1 (auto) or 2 (every store)"), get_knob(&wax_hip_engine::predicate_mirror), FIRST_SHARD},
    {"predicate_mirror_scans", not_set(), get_counter(&wax_hip_engine::st_predicate_mirror_scans), SUM_SHARDS},   // masked scans answered from the bf16 mirror under the certificate
    {"predicate_mirror_fallbacks", not_set(), get_counter(&wax_hip_engine::st_predicate_mirror_fallbacks), SUM_SHARDS},   // ... whose certificate failed: the masked f32 scan answered
    {"predicate_mirror_unavailable", not_set(), get_counter(&wax_hip_engine::st_predicate_mirror_unavailable), SUM_SHARDS},   // ... sent to the f32 scan because the mirror could not be prepared
    {"predicate_batch_rows", set_range(&wax_hip_engine::predicate_batch_rows, 0, 0x7fffffffll, "predicate_batch_rows must be 0..2147483647"), get_knob(&wax_hip_engine::predicate_batch_rows), FIRST_SHARD},
    {"predicate_batch_queries", not_set(), get_counter(&wax_hip_engine::st_predicate_batch_queries), SUM_SHARDS},   // non-empty predicates answered by the batched gather pass
    {"predicate_batch_classes", not_set(), get_counter(&wax_hip_engine::st_predicate_batch_classes), SUM_SHARDS},   // (list, predicate) entries with a predicate that pass built
    {"attr_uploaded_rows", not_set(), get_counter(&wax_hip_engine::st_attr_uploaded), SUM_SHARDS},   // rows of the attribute columns uploaded so far
    {"attr_device_rows", not_set(), GET_EXPR(e->attr_cap), SUM_SHARDS},   // rows the device columns are allocated for (0 = none)
    {"search_many", set_range(&wax_hip_engine::search_many, 0, 1, "search_many must be 0 or 1"), get_knob(&wax_hip_engine::search_many), FIRST_SHARD},
    {"search_many_max_rows", set_range(&wax_hip_engine::search_many_max_rows, 0, 0xffffffffll, "search_many_max_rows must be 0..4294967295"), get_knob(&wax_hip_engine::search_many_max_rows), FIRST_SHARD},
    {"search_many_pooled", not_set(), get_counter(&wax_hip_engine::st_many_pooled), FIRST_SHARD},   // pairs of wax_hip_search_many answered by its pooled launch. A counter, yet not summed: as found, to be decided
    {"search_many_looped", not_set(), get_counter(&wax_hip_engine::st_many_looped), FIRST_SHARD},   // ... by the single-query search under the call's lock. A counter, yet not summed: as found, to be decided
    {"search_many_masked", not_set(), get_counter(&wax_hip_engine::st_many_masked), FIRST_SHARD},   // ... of the pooled ones: by a masked group (a non-empty predicate evaluated on the device). A counter, yet not summed: as found, to be decided
    {"compact_window_rows", set_range(&wax_hip_engine::compact_window_rows, 0, 0xffffffffll, "compact_window_rows must be 0 (what the bounce buffer holds) .. 4294967295"), get_knob(&wax_hip_engine::compact_window_rows), FIRST_SHARD},
    {"remove_batches", not_set(), get_counter(&wax_hip_engine::st_remove_batches), SUM_SHARDS},   // wax_hip_remove_batch calls that removed rows in one pass
    {"remove_batch_rows", not_set(), get_counter(&wax_hip_engine::st_remove_batch_rows), SUM_SHARDS},   // rows they removed
    {"remove_batch_bytes_written", not_set(), get_counter(&wax_hip_engine::st_remove_batch_bytes), SUM_SHARDS},   // device bytes their passes wrote (bounce writes included)
};
#undef GET_EXPR

const TuningRow* tuning_row(const std::string& k) {
    for (const TuningRow& r : kTuning)
        if (k == r.name) return &r;
    return nullptr;
}
const char* tuning_refusal(const TuningSet& s, int64_t v) {   // the row's message for a value it refuses, null for one it takes
    switch (s.kind) {
        case TuningSet::RANGE: case TuningSet::FN: return v < s.a || v > s.b ? s.refusal : nullptr;
        case TuningSet::ONE_OF: return v != s.a && v != s.b && v != s.c ? s.refusal : nullptr;
        case TuningSet::MASK: return (v & ~s.a) ? s.refusal : nullptr;
        default: return nullptr;
    }
}

}  // namespace

extern "C" {

int wax_hip_set_tuning(wax_hip_engine* e, const char* key, int64_t value) {
    if (!e || !key) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    const std::string k(key);
    if (e->sh) return sh_set_tuning(e, k, value);
    const TuningRow* r = tuning_row(k);
    if (!r || r->set.kind == TuningSet::NONE) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "unknown tuning key '" + k + "'");
    if (const char* refusal = tuning_refusal(r->set, value)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, refusal);
    if (r->set.kind == TuningSet::FN) return r->set.fn(e, value);
    e->*(r->set.knob) = r->set.kind == TuningSet::FLAG ? (int64_t)(value != 0) : value;
    return WAX_HIP_OK;
}

int64_t wax_hip_get_tuning(wax_hip_engine* e, const char* key) {
    if (!e || !key) return -1;
    const std::string k(key);
    if (e->sh) return sh_get_tuning(e, k);
    const TuningRow* r = tuning_row(k);
    if (!r) return -1;
    if (r->get.knob) return (e->*(r->get.knob)).load();
    if (r->get.counter) return (int64_t)(e->*(r->get.counter)).load();
    return r->get.fn ? r->get.fn(e) : -1;
}

int wax_hip_time_scan_kernel(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, uint32_t iters,
                             double* out_avg_ms) {
    if (!e || !out_avg_ms || !query) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    SHARDED_UNSUPPORTED(e, "wax_hip_time_scan_kernel");
    if (dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));
    if (iters == 0) iters = 1;
    DeviceGuard g(e->device);
    e->lock.lock_shared(holding(e) > 0);
    { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) { e->lock.unlock_shared(); return frc; } }
    Slot* s = nullptr;
    int rc = WAX_HIP_OK;
    do {
        if (e->count == 0) { rc = fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is empty"); break; }
        const int limit = clamp_topk(top_k);
        const int k_eff = (uint64_t)limit < e->count ? limit : (int)e->count;
        if (k_eff > FUSED_MAX_K) { rc = fail(WAX_HIP_ERR_INVALID_ARGUMENT, "time_scan_kernel: top_k must be <= 192"); break; }
        rc = take_slot(e, &s);
        if (rc != WAX_HIP_OK) break;
        std::memcpy(s->h_query, query, (size_t)dims * sizeof(float));
        ScanArgs a{};
        a.store = e->d_store; a.query = s->d_query; a.partials = s->d_partials; a.dist_out = nullptr;
        a.n_rows = (uint32_t)e->count; a.row_base = (uint32_t)e->row_base; a.dims = e->dims; a.k = k_eff;
        a.q_norm = query_norm(query, dims);
        const int cap = wave_list_cap(k_eff);
        hipError_t err = hipMemcpyAsync(s->d_query, s->h_query, (size_t)dims * sizeof(float), hipMemcpyHostToDevice, s->stream);
        int grid = 0;
        for (int wu = 0; wu < 2 && err == hipSuccess; ++wu)
            err = launch_scan(a, e->metric, (int)e->variant.load(), cap, false, (int)e->grid_blocks.load(), s->stream, &grid);
        if (err == hipSuccess) err = hipEventRecord(s->ev0, s->stream);
        for (uint32_t i = 0; i < iters && err == hipSuccess; ++i)
            err = launch_scan(a, e->metric, (int)e->variant.load(), cap, false, (int)e->grid_blocks.load(), s->stream, &grid);
        if (err == hipSuccess) err = hipEventRecord(s->ev1, s->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(s->stream);
        float ms = 0.f;
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, s->ev0, s->ev1);
        if (err != hipSuccess) { rc = fail(WAX_HIP_ERR_INTERNAL, std::string("time_scan_kernel: ") + hipGetErrorString(err)); break; }
        *out_avg_ms = (double)ms / (double)iters;
    } while (0);
    if (s) e->slots.release(s);
    e->lock.unlock_shared();
    return rc;
}

int wax_hip_time_stream_read(wax_hip_engine* e, uint32_t iters, double* out_avg_ms) {
    if (!e || !out_avg_ms) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    SHARDED_UNSUPPORTED(e, "wax_hip_time_stream_read");
    if (iters == 0) iters = 1;
    DeviceGuard g(e->device);
    e->lock.lock_shared(holding(e) > 0);
    { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) { e->lock.unlock_shared(); return frc; } }
    Slot* s = nullptr;
    int rc = WAX_HIP_OK;
    do {
        const uint64_t bytes = (e->count * (uint64_t)e->dims * 4ull) & ~15ull;
        if (bytes == 0) { rc = fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is empty"); break; }
        rc = take_slot(e, &s);
        if (rc != WAX_HIP_OK) break;
        int grid = (int)e->grid_blocks.load();
        if (grid <= 0) grid = 2048;
        if (grid > MAX_GRID_BLOCKS) grid = MAX_GRID_BLOCKS;
        const int nt = (int)e->stream_nt.load();
        hipError_t err = hipSuccess;
        for (int wu = 0; wu < 2 && err == hipSuccess; ++wu) err = launch_stream_read(e->d_store, bytes, nt, grid, e->d_sink, s->stream);
        if (err == hipSuccess) err = hipEventRecord(s->ev0, s->stream);
        for (uint32_t i = 0; i < iters && err == hipSuccess; ++i) err = launch_stream_read(e->d_store, bytes, nt, grid, e->d_sink, s->stream);
        if (err == hipSuccess) err = hipEventRecord(s->ev1, s->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(s->stream);
        float ms = 0.f;
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, s->ev0, s->ev1);
        if (err != hipSuccess) { rc = fail(WAX_HIP_ERR_INTERNAL, std::string("time_stream_read: ") + hipGetErrorString(err)); break; }
        *out_avg_ms = (double)ms / (double)iters;
    } while (0);
    if (s) e->slots.release(s);
    e->lock.unlock_shared();
    return rc;
}


// Diagnostic read-out of the 8-bit code mirror as the device holds it (tests/test_mirror8_edges_gpu.py): a copy, never a build or a
// refresh, no counter and no breaker state touched. Refused unless the code mirror is valid, so it never hands out rows that are not coded.
int wax_hip_mirror8_snapshot(wax_hip_engine* e, uint64_t first_row, uint64_t n_rows, uint8_t* out_codes, float* out_meta,
                             float* out_max_norm, uint64_t* out_rows_coded) {
    if (!e || !out_max_norm || !out_rows_coded || (n_rows > 0 && (!out_codes || !out_meta))) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    SHARDED_UNSUPPORTED(e, "wax_hip_mirror8_snapshot");
    DeviceGuard g(e->device);
    ReadGuard rg(e);
    BatchMirror& b = e->batch;
    std::unique_lock<std::mutex> mg(b.mu8);
    if (!e->derived.codes.current() || b.d_c8 == nullptr || b.d_c8_meta == nullptr || b.d_c8_max == nullptr || b.c8_cap < e->capacity)
        return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror8_snapshot: the code mirror is absent or not valid");
    const uint64_t rows = e->derived.codes.rows();
    if (first_row > rows || n_rows > rows - first_row)
        return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror8_snapshot: rows [" + std::to_string(first_row) + ", " + std::to_string(first_row) + " + " +
                                                  std::to_string(n_rows) + ") exceed the " + std::to_string(rows) + " coded rows");
    if (b.ev8_pending) HIP_TRY(hipEventSynchronize(b.ev8_ready), WAX_HIP_ERR_INTERNAL, "code mirror ready wait");
    const size_t D = e->dims;
    unsigned int max_bits = 0u;
    HIP_TRY(hipMemcpy(&max_bits, b.d_c8_max, sizeof(max_bits), hipMemcpyDeviceToHost), WAX_HIP_ERR_INTERNAL, "mirror8_snapshot copy");
    if (n_rows > 0) {
        // the device holds 16-row tiles in operand order (mirror8_layout.h); the caller gets rows: the tiles of the range come over as
        // they are, a few thousand at a time, and every 16-byte unit is put where its row has it
        constexpr uint64_t CHUNK_ROWS = 4096 * MIRROR8_TILE_ROWS;
        std::vector<uint8_t> tiles;
        for (uint64_t row0 = first_row / MIRROR8_TILE_ROWS * MIRROR8_TILE_ROWS; row0 < first_row + n_rows; row0 += CHUNK_ROWS) {
            const uint64_t lo = std::max(row0, first_row), hi = std::min(row0 + CHUNK_ROWS, first_row + n_rows);
            tiles.resize(mirror8_bytes(hi - row0, (uint32_t)D));
            HIP_TRY(hipMemcpy(tiles.data(), b.d_c8 + mirror8_offset(row0, 0, (uint32_t)D), tiles.size(), hipMemcpyDeviceToHost), WAX_HIP_ERR_INTERNAL, "mirror8_snapshot copy");
            for (uint64_t r = lo; r < hi; ++r)
                for (uint32_t el = 0; el < D; el += 16)
                    std::memcpy(out_codes + (r - first_row) * D + el, tiles.data() + mirror8_offset(r - row0, el, (uint32_t)D), 16);
        }
        HIP_TRY(hipMemcpy(out_meta, b.d_c8_meta + 2 * first_row, (size_t)n_rows * 2 * sizeof(float), hipMemcpyDeviceToHost), WAX_HIP_ERR_INTERNAL, "mirror8_snapshot copy");
    }
    std::memcpy(out_max_norm, &max_bits, sizeof(float));
    *out_rows_coded = rows;
    return WAX_HIP_OK;
}

// Diagnostic read-out of the keys of the 8-bit pass (tests/test_mirror8_mfma_gpu.py): the lower bound the lone scan computes for
// `query` at every coded row, by the scan's own body. Like the snapshot: never a build or a refresh, no counter and no breaker state
// touched, refused unless the code mirror is valid. No product path calls it.
int wax_hip_mirror8_keys(wax_hip_engine* e, const float* query, float* out_keys, uint64_t n_keys) {
    if (!e || !query || !out_keys) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    SHARDED_UNSUPPORTED(e, "wax_hip_mirror8_keys");
    DeviceGuard g(e->device);
    ReadGuard rg(e);
    BatchMirror& b = e->batch;
    std::unique_lock<std::mutex> mg(b.mu8);
    if (!e->derived.codes.current() || b.d_c8 == nullptr || b.d_c8_meta == nullptr || b.d_c8_max == nullptr || b.c8_cap < e->capacity)
        return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror8_keys: the code mirror is absent or not valid");
    const uint64_t rows = e->derived.codes.rows();
    if (rows == 0 || rows > e->count || n_keys != rows)
        return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror8_keys: out_keys holds " + std::to_string(n_keys) + " keys, the code mirror " + std::to_string(rows) + " rows");
    if (!mirror_scan_supported(e->dims, e->metric)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror8_keys: no 8-bit pass at this dimension and metric");
    if (b.ev8_pending) HIP_TRY(hipEventSynchronize(b.ev8_ready), WAX_HIP_ERR_INTERNAL, "code mirror ready wait");
    MirrorScanArgs m{};
    m.n_rows = (uint32_t)rows;
    m.row_base = (uint32_t)e->row_base;
    m.dims = e->dims;
    m.k = 1;
    m.kpad = 1;
    m.q_norm = query_norm(query, e->dims);
    float* d_keys = nullptr;
    HIP_TRY(hipMalloc(&d_keys, (size_t)rows * sizeof(float)), WAX_HIP_ERR_INTERNAL, "mirror8_keys allocation");
    hipError_t err = launch_mirror8_keys(m, b.d_c8, b.d_c8_meta, query, e->metric, (int)e->grid_blocks.load(), d_keys, nullptr);
    if (err == hipSuccess) err = hipMemcpy(out_keys, d_keys, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d_keys);
    HIP_TRY(err, WAX_HIP_ERR_INTERNAL, "mirror8_keys");
    return WAX_HIP_OK;
}

// Diagnostic for tests/test_mirror_gap_gpu.py: the mirror finish's choice of its MIRROR_KP approximate candidates, both ways, on lists
// the caller makes up (launch_mirror_select_probe). No engine, no product path.
int wax_hip_mirror_select_probe(const int64_t* lists, uint32_t n_lists, int64_t* out_selected, int64_t* out_merged, int32_t* out_gathered) {
    if (!lists || !out_selected || !out_merged || !out_gathered) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (n_lists < 1 || n_lists > (uint32_t)SCAN_KWAY_MERGE_GRID) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror_select_probe: 1 to 512 lists");
    const size_t in_bytes = (size_t)n_lists * MIRROR_KP * sizeof(int64_t), out_bytes = 2 * (size_t)MIRROR_KP * sizeof(int64_t);
    char* d = nullptr;
    HIP_TRY(hipMalloc(&d, in_bytes + out_bytes + sizeof(int)), WAX_HIP_ERR_INTERNAL, "mirror_select_probe allocation");
    int64_t* d_out = reinterpret_cast<int64_t*>(d + in_bytes);
    int* d_gathered = reinterpret_cast<int*>(d + in_bytes + out_bytes);
    int64_t host_out[2 * MIRROR_KP];
    int gathered = 0;
    hipError_t err = hipMemcpy(d, lists, in_bytes, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = launch_mirror_select_probe(reinterpret_cast<const int64_t*>(d), (int)n_lists, d_out, d_gathered, nullptr);
    if (err == hipSuccess) err = hipMemcpy(host_out, d_out, out_bytes, hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(&gathered, d_gathered, sizeof(int), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIP_TRY(err, WAX_HIP_ERR_INTERNAL, "mirror_select_probe");
    std::memcpy(out_selected, host_out, out_bytes / 2);
    std::memcpy(out_merged, host_out + MIRROR_KP, out_bytes / 2);
    *out_gathered = gathered;
    return WAX_HIP_OK;
}

// Diagnostic for tests/test_pass_lists_gpu.py: the selection frame of a mirror pass on keys the caller makes up
// (launch_mirror_lists_probe). No engine, no product path.
int wax_hip_mirror_lists_probe(const int64_t* keys, uint32_t nq, uint64_t n_slots, uint32_t grid, int64_t* out_partials) {
    if (!keys || !out_partials) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (nq < 1 || nq > (uint32_t)MIRROR_MAX_NQ) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror_lists_probe: 1 to 4 queries");
    if (grid < 1 || grid > 8) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror_lists_probe: 1 to 8 workgroups");
    if (n_slots < 1 || n_slots > (1ull << 24)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "mirror_lists_probe: 1 to 2^24 slots");
    const size_t in_bytes = (size_t)nq * n_slots * sizeof(int64_t), out_bytes = (size_t)nq * grid * MIRROR_KP * sizeof(int64_t);
    char* d = nullptr;
    HIP_TRY(hipMalloc(&d, in_bytes + out_bytes), WAX_HIP_ERR_INTERNAL, "mirror_lists_probe allocation");
    int64_t* d_out = reinterpret_cast<int64_t*>(d + in_bytes);
    hipError_t err = hipMemcpy(d, keys, in_bytes, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = launch_mirror_lists_probe(reinterpret_cast<const int64_t*>(d), (int)nq, (uint32_t)n_slots, (int)grid, d_out, nullptr);
    if (err == hipSuccess) err = hipMemcpy(out_partials, d_out, out_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIP_TRY(err, WAX_HIP_ERR_INTERNAL, "mirror_lists_probe");
    return WAX_HIP_OK;
}
