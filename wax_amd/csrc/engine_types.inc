// engine_types.inc — part of engine.hip's translation unit (included there; not compiled alone).
// types of the host side: error state, the device guard, scratch slots, workspaces, the bf16 mirror's bookkeeping, `struct wax_hip_engine`, ticket ownership

namespace {

thread_local std::string g_last_error;


int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

#define HIP_TRY(expr, code, what)                                                         \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return fail((code), std::string(what) + ": " + hipGetErrorString(_e));        \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) {
            changed = (hipSetDevice(dev) == hipSuccess);
        }
    }
    ~DeviceGuard() {
        if (changed && prev >= 0) (void)hipSetDevice(prev);
    }
};

constexpr int kShardRing = 8;

// A scan's stage buffer: per-workgroup partial top-k lists, followed by one cache line holding the arrival ticket of the
// fused final merge (scan_epilogue: zero between launches — the last arriver re-arms it).
constexpr size_t kPartialsBytes = (size_t)MAX_GRID_BLOCKS * FUSED_MAX_K * sizeof(int64_t) + 128;
// the mirror scan's certificate word: in the slot's pinned 64-byte completion block, behind the completion word
inline uint32_t* slot_cert_word(uint64_t* h_done) { return reinterpret_cast<uint32_t*>(h_done + 2); }
inline uint32_t* partials_ticket(int64_t* d_partials) {
    return reinterpret_cast<uint32_t*>(d_partials + (size_t)MAX_GRID_BLOCKS * FUSED_MAX_K);
}

constexpr int kMaxStreams = 4;
constexpr int kHardSlotCap = 256;        // scratch slots a thread that pipelines submits without collecting can bring the pool to (work_pool.h)
constexpr size_t kPredCounts = 3;        // words of FilterWork::d_pred_counts and PredEntry::d_counts (AttrMaskArgs::counts)

struct Slot {
    int index = 0;
    hipStream_t stream = nullptr;  // one of the engine's streams (not owned)
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_done = nullptr;
    uint64_t* h_done = nullptr;    // pinned: the completion word a fused scan publishes behind its hits ("done_flag")
    bool coherent = false;         // h_hits / h_done are coherent host memory (a condition of the completion-word path)
    uint64_t done_seq = 0;         // value the slot's current query publishes
    bool flag_wait = false;        // this ticket completes through h_done (no event was recorded)
    hipEvent_t t_start = nullptr, t_end = nullptr;   // the events that bracket this ticket's scan kernel (not owned)
    float* d_query = nullptr;
    float* h_query = nullptr;  // pinned
    int64_t* d_partials = nullptr;
    wax_hip_hit* d_hits = nullptr;
    wax_hip_hit* h_hits = nullptr;  // pinned
    // general path, allocated on first use
    float* d_dist = nullptr;
    uint64_t dist_cap = 0;
    SelectWork sw{};
    bool sw_ready = false;
    // per-ticket state
    int k_eff = 0;
    bool timed = false;
    bool mirror = false;           // answered by the mirror scan: collect reads the certificate word and re-runs the f32 scan if it failed
    bool mirror8 = false;          // ... and the mirror it rode was the 8-bit code mirror ("mirror_bits"): its certificate feeds the breaker
    bool want8 = false;            // (parked) this query may ride the code mirror if the set it is launched with takes it
    float q_norm = 0.f;            // (mirror) the query's norm; the query itself is in h_query
    // "mirror_share": this ticket was parked at submit (its query waits in h_query for a pass it can share). `shared` is written before
    // the ticket is published and tells collect to look under the engine's share_mu; the other two are guarded by that mutex.
    bool shared = false;
    bool listed = false;           // launched on the mirror and in the engine's share_launched until its collect ("mirror_fill")
    int park_rc = 0;               // what launching it returned (a failed launch surfaces at the ticket's collect)
    std::string park_err;
    std::thread::id owner;         // the submitting thread (its outstanding-ticket count drops at collect, whoever collects)
    // wax_hip_search_predicate_submit (DESIGN 4.5): the score cut applied at collect; the predicate (normalised, non-empty) of a ticket
    // that rides a masked pass or is deferred to the blocking body, and the bitmap entry it holds a use of (-1: none). `pred_deferred`
    // may be set by the launch of the set the ticket was parked in (share_mu), so collect reads it behind that mutex.
    bool has_cut = false;
    float cut = 0.f;
    bool has_pred = false;
    bool pred_deferred = false;    // answered at collect by the blocking body (search_rows_locked) under the lock the ticket holds
    wax_hip_row_predicate pred{};
    int pred_entry = -1;
    int32_t top_k = 0;             // as the caller gave it (the blocking body clamps it itself)
};

// A row bitmap of one predicate on one state of the store (wax_hip_engine::pred_entries): what the predicate tickets' masked passes
// read. Built on the stream of the first pass that needs it, in front of that pass, without a host synchronisation; its passing-row
// count travels to pinned memory behind the build and is known once `built_ev` has completed.
struct PredEntry {
    wax_hip_row_predicate pred{};
    uint64_t epoch = 0;              // RWLock::epoch() of the store state the bitmap describes
    bool assigned = false;           // pred / epoch are set
    bool built = false;              // the build is enqueued (built_ev recorded on build_stream)
    uint32_t* d_bitmap = nullptr;
    uint64_t words = 0;              // capacity of d_bitmap
    uint32_t* d_counts = nullptr;    // [kPredCounts] attr_mask_kernel's: passing rows, 16-row tiles that hold one
    uint32_t* h_counts = nullptr;    // pinned [kPredCounts]
    hipEvent_t built_ev = nullptr;
    hipStream_t build_stream = nullptr;
    int users = 0;                   // parked or uncollected tickets: an entry in use is never evicted or rebuilt
    uint64_t last_use = 0;
};
constexpr int kPredEntries = 4;

// Workspace of one wax_hip_search_filtered call: pooled (4 per engine, allocated on demand) with its own stream,
// so filtered searches run concurrently with each other and with every other read entry point.
struct FilterWork {
    hipStream_t stream = nullptr;
    uint32_t* d_rows = nullptr;      // [cap] allowed local rows, ascending
    uint64_t* d_ids = nullptr;       // [cap] their frame ids
    float* d_dist = nullptr;         // [cap] their distances
    uint64_t cap = 0;
    uint64_t* d_allow = nullptr;     // [allow_cap] the caller's allow-list (device-side probe)
    uint64_t allow_cap = 0;
    uint32_t* d_bitmap = nullptr;    // [bitmap_words] one bit per store row
    uint64_t bitmap_words = 0;
    uint32_t* d_block_sum = nullptr; // [block_cap] per-block popcounts -> exclusive offsets
    uint64_t block_cap = 0;
    uint32_t* d_total = nullptr;     // [1]
    uint32_t* h_total = nullptr;     // pinned [1]
    float* d_query = nullptr;        // [dims]
    float* d_qnorm = nullptr;        // [1]
    wax_hip_hit* d_hits = nullptr;   // [WAX_HIP_MAX_RESULTS]
    wax_hip_hit* h_hits = nullptr;   // pinned [WAX_HIP_MAX_RESULTS]
    SelectWork sw{};
    // wax_hip_search_batch_filtered (d_allow above holds the caller's packed lists)
    float* d_bq = nullptr;           // [bq_cap] the batch's queries
    uint64_t bq_cap = 0;
    unsigned char* d_meta = nullptr; // [meta_cap] list descriptors, groups, work table, query slots, norms, merge spans (one upload)
    uint64_t meta_cap = 0;
    uint32_t* d_lrows = nullptr;     // [lrows_cap] compact row lists, one region per distinct list
    uint64_t lrows_cap = 0;
    uint32_t* d_lcnt = nullptr;      // [lcnt_cap] their device-side lengths
    uint64_t lcnt_cap = 0;
    uint64_t* d_lids = nullptr;      // [lids_cap] frame ids the bitmap route writes beside its rows: allow_emit needs an id output; never read
    uint64_t lids_cap = 0;
    int64_t* d_part = nullptr;       // [part_cap] per-(query, work item) partial key lists
    uint64_t part_cap = 0;
    wax_hip_hit* d_bhits = nullptr;  // [bhits_cap] merged hits, one row of k per fused query
    uint64_t bhits_cap = 0;
    // wax_hip_search_batch_terms: the term pass in front of the entries' layout
    uint32_t* d_tplan = nullptr;     // [tplan_cap] per launch: union terms | membership words (512 each), then one count per set
    uint64_t tplan_cap = 0;
    uint32_t* d_tbits = nullptr;     // [tbits_cap] one row bitmap per admitted term set
    uint64_t tbits_cap = 0;
    // wax_hip_search_predicate (allocated by its first call on this workspace)
    uint32_t* d_pred_counts = nullptr;   // [kPredCounts] passing rows, scan chunks that hold one, mirror chunks that hold one (attr_mask_kernel)
    uint32_t* h_pred_counts = nullptr;   // pinned [kPredCounts]
    int64_t* d_partials = nullptr;       // masked scan: kPartialsBytes, the per-workgroup lists + the short merge's flag words
    // the masked scan's mirror form ("predicate_mirror"): what mirror_finish_kernel writes — [MIRROR_MAX_K] hits, then one slot whose
    // first word is the certificate — so that one copy brings both to the host
    wax_hip_hit* d_mirror_out = nullptr; // [MIRROR_MAX_K + 1]
    wax_hip_hit* h_mirror_out = nullptr; // pinned [MIRROR_MAX_K + 1]
};

void free_filter_work(FilterWork* f);

// id -> row table in HBM (filter.hip): built at the first long allow-list, brought up to date lazily after a mutation. How far it has
// followed the store is DerivedRows::idtable (derived_rows.h): appends insert rows [rows, count), a removal or a deserialize starts it
// over (like the reference's firstIndex(of:) scan they are O(N) anyway).
struct IdHash {
    std::mutex mu;                   // serialises the (re)build only
    uint32_t* d_table = nullptr;
    uint64_t slots = 0;
};

// Batched (bf16 MFMA) path. The corpus mirror is shared by every batch (read-only during searches, rebuilt lazily by
// the first batch after a mutation); everything a call writes lives in a pooled per-call workspace with its own
// stream, so batched searches run concurrently with each other like every other read entry point.
struct BatchMirror {
    std::mutex mu;                       // serialises the (re)build only
    unsigned short* d_cb = nullptr;      // [mirror_cap][dims] bf16 (cosine rows pre-normalised)
    float* d_vn2 = nullptr;              // [mirror_cap] ||v||^2
    unsigned int* d_maxnorm = nullptr;
    uint64_t mirror_cap = 0;
    // A mutation does not throw the mirror away (re-converting the WHOLE store after any add / remove is 30.7 GB read + 15.4 GB written
    // and a blocking sync at 10M x 768, per mutation, on an ingest-while-serving workload — the reference's add is one row copy,
    // MetalVectorEngine.swift:330-357): what each mutation leaves to convert is DerivedRows::bf16 (derived_rows.h); only reallocation
    // without the old contents and deserialize convert everything again.
    // max ||v|| and max ||x - bf16(x)|| stay on the device (d_maxnorm, read there by the prep kernel) and only ever grow between full
    // conversions: a bound that is too large by a row that has since been overwritten or removed is still a bound.
    uint32_t* d_dirty = nullptr;         // [kMirrorMaxDirty] the overwritten rows of a listed-rows conversion
    hipEvent_t ev_ready = nullptr;       // recorded behind the last conversion: other workspaces' streams wait for it
    bool ev_pending = false;
    std::atomic<uint64_t> rows_converted{0}, conversions{0};   // statistics ("mirror_rows_converted" / "mirror_conversions")
    // The 8-bit code mirror of the single-query scan (mirror8_scan.hip; DESIGN 4.1): codes + 128 and {scale, err} per row, built from
    // the f32 store. Maintenance is deliberately simpler than the bf16 mirror's (DerivedRows::codes): appends convert rows [rows, count);
    // every other mutation and a reallocation start it over, and a code mirror that has to start over is rebuilt only when three
    // eligible queries in a row since the last mutation wanted it — until then they take bf16.
    std::mutex mu8;                      // serialises the (re)build only
    unsigned char* d_c8 = nullptr;       // biased codes in 16-row tiles, MFMA operand order (mirror8_layout.h): ceil16(c8_cap) * dims bytes
    float* d_c8_meta = nullptr;          // [c8_cap] float2 {scale, err}
    unsigned int* d_c8_max = nullptr;    // one word: max ||v|| over the coded rows (grows between full conversions, like d_maxnorm)
    uint64_t c8_cap = 0;
    hipEvent_t ev8_ready = nullptr;      // recorded behind the last conversion: other slots' streams wait for it
    bool ev8_pending = false;
    std::atomic<uint64_t> rows8_converted{0}, conversions8{0};   // "mirror8_rows_converted" / "mirror8_conversions"
};

constexpr int kBreakerWindow = 32, kBreakerFails = 8, kBreakerHold = 1024;   // "mirror_bits" breaker (wax_hip_engine::breaker_*)
constexpr uint32_t kBatchMaxQ = 1024;   // queries per GEMM pass
constexpr uint32_t kBatchSegBase = FUSED_MAX_K;   // slab pipeline: a candidate row = [0, kBatchSegBase) best list, then the survivor area
constexpr uint32_t kBatchSegArea = 4096;          // survivors per query between two tighten passes (slab pipeline) / of the one pass
constexpr uint32_t kBatchCandCap = kBatchSegBase + kBatchSegArea;
constexpr uint32_t kBatchMaxSegs = 256;           // GEMM workgroups per query group
constexpr uint32_t kBatchFirstSlab = 2048;  // rows of the first slab (everything passes: tau = +inf)
constexpr int kBatchMaxKSlab = 80;      // largest k served by the slab pipeline (k' = 2k+32 <= 192)
constexpr int kBatchMaxK = 464;         // largest k served by the one-pass pipeline (k' = 2k+32 <= 960): covers the real caller's
                                        // candidateLimit = max(topK, min(3 topK, 1000)) up to topK 154 (UnifiedSearch.swift:1195-1200)

struct BatchCtx {
    hipStream_t stream = nullptr;        // owned
    hipEvent_t ev_in = nullptr;          // caller-stream -> ctx-stream ordering for device-resident inputs
    hipEvent_t ev_g0 = nullptr, ev_g1 = nullptr;   // "time_kernels": around the filtering GEMM of the last enqueued block
    hipEvent_t ev_gc = nullptr;                    // "time_kernels" = 2: the chain event behind it (ev_g0 / ev_g1 are bound to the dispatch)
    bool gemm_timed = false;
    uint32_t gemm_rows = 0, gemm_queries = 0;
    float* d_q = nullptr;                // [q_cap][dims] staging for host queries
    uint64_t q_cap = 0;
    unsigned short* d_qb = nullptr;
    unsigned short* d_qf = nullptr;                // the same queries in MFMA A-fragment order (GemmArgs::qf)
    float* d_qn2 = nullptr;
    float* d_qnorm = nullptr;
    float* d_eps = nullptr;
    float* d_tau = nullptr;              // [kBatchMaxQ] admission thresholds
    float* d_dense = nullptr;            // slab pipeline: [kBatchMaxQ][kBatchFirstSlab] first-slab score tile
    uint32_t* d_cand_count = nullptr;
    uint32_t* d_overflow = nullptr;
    int64_t* d_cand = nullptr;           // [rows of a block][slots per query]; cand_slots = capacity in keys
    uint64_t cand_slots = 0;
    uint32_t* d_seg_count = nullptr;     // [kBatchMaxSegs][kBatchMaxQ] survivors per (GEMM workgroup, query)
    int64_t* d_exact = nullptr;          // [kBatchMaxQ][kp_cap]
    int64_t* d_sel = nullptr;            // [kBatchMaxQ][kp_cap] (one-pass pipeline, k' > 192)
    uint64_t kp_cap = 0;
    float* d_tile_max = nullptr;         // one-pass pipeline: [tile_max_rows][kBatchMaxQ]
    uint64_t tile_max_rows = 0;
    wax_hip_hit* d_hits = nullptr;       // [hits_cap] hits of a whole host-pointer call
    uint64_t hits_cap = 0;
    uint64_t cert_cap = 0;
    wax_hip_hit* h_hits = nullptr;       // pinned [hits_cap]
    // full retry of uncertified queries (single-block one-pass batches): the finish arguments of the last block, the failed
    // queries' numbers (pinned + device)
    FinishArgs last_finish{};
    int last_metric = 0;
    bool last_finish_valid = false;
    uint32_t* h_qlist = nullptr;         // pinned [kBatchMaxQ]
    uint32_t* d_qlist = nullptr;         // [kBatchMaxQ]
    // shared exact pass over the uncertified queries (multiscan.hip): their norms by slot, per-(query, workgroup) partial top-k
    float* h_fnorm = nullptr;            // pinned [kBatchMaxQ]
    float* d_fnorm = nullptr;            // [kBatchMaxQ]
    int64_t* d_mpart = nullptr;          // [group][grid][k]
    uint64_t mpart_cap = 0;
    int64_t* d_rescue = nullptr;         // full retry: [queries of a round][survivor area] dense survivor keys
    uint64_t rescue_cap = 0;
    int64_t* d_rescue_exact = nullptr;   // full retry: [queries of a round][largest live count] their exact keys
    uint64_t rescue_exact_cap = 0;
    uint32_t* h_live = nullptr;          // pinned [kBatchMaxQ]: live survivors per query of a retry round
    uint32_t* h_cert = nullptr;          // pinned [cert_cap]
    uint32_t* d_cert = nullptr;          // device [cert_cap]: the finish kernel's flags for the device-side retry kernel
    float* h_qnorm = nullptr;            // pinned [cert_cap]: exact norms (the exact-path fallback needs them on the host)
};

struct ShardedState;   // sharded.inc: the multi-GPU handle's state (null for a single-device engine)

}  // namespace

struct wax_hip_engine {
    ShardedState* sh = nullptr;
    int device = 0;
    uint8_t metric = 0;
    uint32_t dims = 0;
    uint64_t count = 0;           // vectorCount
    uint64_t capacity = 0;        // reservedCapacity, rows
    float* d_store = nullptr;     // [capacity][dims]
    uint64_t* d_ids = nullptr;    // [capacity]
    std::vector<uint64_t> ids;    // frameIds (host mirror; row order)
    IdMap idmap;
    uint64_t row_base = 0;
    RWLock lock;

    hipStream_t streams[kMaxStreams] = {};
    std::atomic<int> n_streams{2};   // slots are spread round-robin over this many in-order streams
    // Scan kernels are chained across streams through this event so that they never overlap each
    // other (each one owns the whole HBM pipe and its HIP-event duration stays meaningful) while
    // the merge kernel, the query upload and the result write of neighbouring queries do overlap.
    hipEvent_t scan_done = nullptr;
    hipEvent_t chain_event = nullptr;  // event the next chained scan waits on: scan_done or the last scan's end-of-kernel timing event
    bool scan_done_valid = false;
    // End-of-kernel timing events of chained scans come from this ring (not from the slot): the end of scan i is also
    // the START of scan i+1 when i is still in flight at i+1's submit, so only two packets (record, wait) sit between
    // two scans instead of three. A ring entry is re-recorded kTimingRing chained scans later — more than the
    // kHardSlotCap tickets that can be outstanding — so both tickets that read it have been collected by then.
    static constexpr int kTimingRing = 1024;
    hipEvent_t tev[kTimingRing] = {};
    uint32_t tev_next = 0;
    bool chain_is_timing = false;
    std::atomic<int64_t> share_timing{1};
    // Pipelined scans of different streams: 1 = chained through an event (they never overlap: a per-launch HIP-event
    // duration is one scan alone), 0 = free to overlap (no idle HBM between two scans, ramp and tail of neighbouring
    // kernels hidden: +3 .. +19 % queries/s), -1 (default) = chained exactly when the kernels are being timed
    // ("time_kernels" = 1), so the product path is the fast one and a measurement pass still gets clean per-launch times.
    std::atomic<int64_t> scan_chain{-1};
    std::mutex chain_mu;

    // The scratch slots, the batch workspaces and the filtered-search workspaces (work_pool.h: who waits, who is refused, who grows), the
    // tickets in flight, and the uncollected tickets per submitting thread (rw_lock.h).
    WorkPool<Slot> slots{4, kHardSlotCap};
    TicketTable<Slot*> tickets;
    TicketHolders holders;

    // shard-search scratch ring (caller-stream async work)
    float* ring_d_query[kShardRing] = {};
    float* ring_h_query[kShardRing] = {};
    int64_t* ring_d_partials[kShardRing] = {};
    hipEvent_t ring_ev0[kShardRing] = {}, ring_ev1[kShardRing] = {};
    hipEvent_t ring_t0[kShardRing] = {}, ring_t1[kShardRing] = {};   // the events that bracket the entry's scan (not owned)
    bool ring_ev_pending[kShardRing] = {};
    // Completion of everything the entry's last use enqueued on the caller's stream (query upload, scan, merge):
    // waited for before the entry is reused (its pinned query and partials are still being read until then) and by
    // every writer (the caller-stream work runs after the shared lock was released).
    hipEvent_t ring_done[kShardRing] = {};
    bool ring_busy[kShardRing] = {};
    std::mutex ring_mu[kShardRing];
    std::atomic<uint32_t> ring_next{0};
    // wax_hip_timeline_device's scratch (api_timeline.inc): the partial lists of a launch on the CALLER's stream, in use until `done`
    // (recorded behind the launch) has passed; `cols` orders the caller's stream behind the attribute upload. Entries are taken in
    // turn, one user at a time, and waited for by every writer like the shard ring above.
    struct TimelineRing {
        std::mutex mu;
        int64_t* d = nullptr;
        uint64_t words = 0;
        hipEvent_t done = nullptr, cols = nullptr;
        bool busy = false;
    } tl_ring[kShardRing];
    std::atomic<uint32_t> tl_next{0};

    float* d_sink = nullptr;
    void* d_bounce = nullptr;
    // wax_hip_remove_batch (DESIGN 4.7)
    std::atomic<int64_t> compact_window_rows{0};   // source rows per window of the compaction pass; 0 = what the bounce buffer holds
    std::atomic<uint64_t> st_remove_batches{0}, st_remove_batch_rows{0}, st_remove_batch_bytes{0};

    // tuning
    std::atomic<int64_t> grid_blocks{0};
    std::atomic<int64_t> variant{-1};
    std::atomic<int64_t> time_kernels{0};
    std::atomic<int64_t> force_general{0};
    std::atomic<int64_t> select_grid{0};     // workgroups of the radix selection's histogram and compaction passes: 0 = min(2048, ceil(rows / 256)), else at most this many (1..2048; tests drive the multi-trip loops on small stores)
    std::atomic<int64_t> select_short{1};    // k > 192: select from the fused scan's per-workgroup lists first (one launch, certified); 0 = the distance pass + radix selection at once
    std::atomic<int64_t> stream_nt{1};
    std::atomic<int64_t> scan_plain_mb{32};  // single-query scans with the query in their arguments: stores up to this many MB read their rows with ordinary loads (-1 = grids <= 160 workgroups)
    std::atomic<int64_t> merge_kway{1};      // fused final merge, k <= 64: 1 (default) = k-way merge of the per-workgroup lists' heads; 0 = stream them through the wave lists
    std::atomic<int64_t> done_flag{1};       // single-query scans that merge in the kernel publish a completion word in pinned memory; collect polls it instead of an event (0 = always an event)
    std::atomic<uint64_t> st_flag_waits{0};
    std::atomic<int64_t> query_args{1};      // single-query scans: 1 (default) = stores whose scan grid is small enough for the fused merge (the launch-latency-bound ones) get the query in the kernel arguments (no upload copy); 2 = every store; 0 = always upload
    std::atomic<int64_t> fuse_merge{1};      // 1 = grids of <= SCAN_FUSE_MERGE_GRID workgroups merge in the scan kernel's last-arriving workgroup
    // A scan submitted while other tickets of this engine are still out (a caller that keeps several queries in flight, or several
    // callers at once) runs in a stream of scans: there the separate merge launch overlaps the NEXT scan, while the last arriver's
    // tail (ticket, k-way merge, id gather, ~8 us) is serial inside the kernel. Stores of at least this many MB then take the
    // two-launch form (upload, scan, merge; 0 = never). A query submitted alone keeps the single launch (12 - 14 us less latency).
    // Pipelined, depth 4, 384-d (profiles/r05/k_pipelined_merge_forms.txt): 100K rows 24.8 us per query in one launch against 30.1
    // in two, 200K 45.3 / 45.6, 400K 88.9 / 87.0, 700K 154.0 / 150.1, 1M 224.3 / 214.3, 1.25M 274.3 / 268.7.
    std::atomic<int64_t> merge_overlap_mb{400};
    std::atomic<uint64_t> st_overlap_scans{0};
    std::atomic<uint64_t> st_short_selects{0};   // short selections enqueued by enqueue_scan (k > 192 in front of the radix selection; 64 < k <= 192 in front of the second-launch merge)
    std::atomic<int64_t> batch_qfrag{1};     // 1 (default) = the prep kernel also writes the bf16 queries in MFMA A-fragment order and the register-resident GEMM loads them from there (coalesced); 0 = row-major reads
    std::atomic<int64_t> batch_min{1};       // fewer queries than this: always pipelined single-query scans (1..15: cost model below)
    std::atomic<int64_t> batch_mode{1};      // 0 = never use the MFMA path
    std::atomic<int64_t> batch_slab_mb{64};  // cap on slab size, in units of 16 384 rows
    std::atomic<int64_t> batch_growth{8};    // next slab = growth x rows seen so far
    std::atomic<int64_t> batch_first{2048};  // rows of the dense first slab (<= kBatchFirstSlab)
    std::atomic<int64_t> batch_prof_ptr{0};  // diagnosis: device address of the phase-timing buffer of the filtering GEMM (GemmArgs::prof); 0 = the product kernel
    std::atomic<int64_t> batch_debug{0};     // test / diagnosis bits, none of which can change an answer: 4096 = no pace gate, 16384 = one wave of workgroup 1 pretends its split-barrier wait timed out, 65536 = the device-side retry re-scores every survivor
    std::atomic<int64_t> batch_dyn_tail{1};  // the filtering GEMM's last tiles are claimed from a pool instead of walked in fixed shares (0 = fixed shares)
    std::atomic<int64_t> batch_host_multi{1};   // host-pointer batches the MFMA pipelines do not take: 1 (default) = shared exact passes, 16 queries per pass; 0 = one scan per query
    std::atomic<int64_t> batch_in_wait{0};   // device-resident batches: 1 = always order the workspace's stream behind the caller's with an event; 0 (default) = only while the caller's stream has work pending
    std::atomic<int64_t> batch_rega{1};      // register-resident-queries GEMM where it applies: 1 (default) workgroup barrier per tile, 5 split tile barrier; 0 = the LDS-tiled kernel instead
    std::atomic<uint64_t> st_batch_queries{0}, st_batch_fallbacks{0}, st_idhash_rows{0};
    BatchMirror batch;
    WorkPool<BatchCtx> bctxs{4};
    std::atomic<int64_t> batch_onepass{1};        // 0 = always the slab pipeline
    std::atomic<int64_t> batch_onepass_tiles{64};     // smallest store (in units of 64 rows, 32 at D = 768) the one-pass pipeline takes (rounds 2-5: 1024; measured down to 64: profiles/r06/r_*)
    std::atomic<int64_t> batch_survivors{3};      // one-pass pipeline: expected survivors per query = this x k'
    std::atomic<int64_t> batch_kp_fused{1};       // one-pass pipeline, k in 81 .. 128: 1 = k' capped at 192 (fused finish kernel + device retry); 0 = k' = 2k + 32 (three-launch finish)
    std::atomic<int64_t> batch_retry{1};          // one-pass pipeline: uncertified queries get a full retry (ALL their survivors re-scored) before the exact path
    std::atomic<int64_t> batch_multi{1};          // exact path of a batch: 1 = uncertified queries share passes over the f32 store (multiscan.hip), 0 = one scan each
    std::atomic<uint64_t> st_multi_passes{0}, st_multi_queries{0};
    std::atomic<uint64_t> st_batch_retries{0};
    std::atomic<int64_t> batch_sample_div{32};    // one-pass pipeline: 1 / this of the tiles are sampled (at least 256)
    std::atomic<uint64_t> st_onepass_queries{0};
    std::atomic<int64_t> batch_eps_measured{1};       // cosine certificate bound from the MEASURED bf16 rounding errors (per query, max over rows) instead of the worst case
    std::atomic<int> retry_hint{0};                   // > 0: batches carry the device-side retry kernel behind their finish kernel
    std::atomic<uint64_t> st_batch_inline_retries{0};  // ... of which inside the finish kernel (no host round trip)
    std::atomic<uint64_t> st_merged_scans{0};        // single-query scans whose last-arriving workgroup did the final merge (one launch per query)
    std::atomic<uint64_t> st_query_args{0};          // single-query scans that took their query through the kernel arguments
    std::atomic<int64_t> scan_mirror{1};     // single queries on the bf16 mirror + f32 re-score + certificate: 1 (default) = stores of > SCAN_KWAY_MAX_BYTES of rows, 2 = always, 0 = never
    std::atomic<uint64_t> st_mirror_scans{0}, st_mirror_fallbacks{0}, st_mirror_unavailable{0};
    // Single queries in flight share passes over the mirror ("mirror_share": 0 = never, 1 (default) = a query submitted while a mirror
    // pass of this engine is still running is parked and launched with the others parked by then, 2 = always parked until a collect
    // needs the answer or the group is full). Any thread may launch what another parked: the parked set, and every launch of a
    // mirror pass that looks at it, is behind share_mu.
    std::atomic<int64_t> mirror_share{1};
    std::mutex share_mu;
    std::vector<Slot*> parked;               // submit order; at most MIRROR_MAX_NQ - 1 between two calls
    std::atomic<int> n_parked{0};            // parked.size(), readable without the mutex
    hipEvent_t share_last = nullptr;         // ev_done of the last mirror pass launched (a slot's event: not owned); not ready = a pass in flight
    std::atomic<uint64_t> st_mirror_passes{0}, st_mirror_shared_passes{0}, st_mirror_shared_queries{0};
    // "mirror_fill" (1 = default): under "mirror_share" 1 a caller who pipelines single queries gets full passes. Mirror tickets that
    // are launched and not yet collected are a pass in flight or, finished, mean that their caller is draining a pass and its next
    // submits are on the way: a submit that finds such tickets is parked, and neither it nor a collect that blocks on a running
    // ticket launches a set that is not full. 0 = the eager rule (a blocking collect and a submit without a pass in flight launch
    // whatever is parked).
    std::atomic<int64_t> mirror_fill{1};
    std::vector<Slot*> share_launched;       // mirror tickets launched and not yet collected (share_mu); no event of a parked slot is ever asked
    std::atomic<uint64_t> st_mirror_fill_holds{0};   // submits parked or held by the rule + blocking collects that held the set back
    // "mirror_bits": which mirror a single query that takes one streams. 0 (default) = auto: the 8-bit code mirror for k <= MIRROR8_MAX_K
    // where "scan_mirror" is 1 and the store is above SCAN_KWAY_MAX_BYTES, else bf16; 8 = the code mirror wherever a mirror is taken
    // (k <= MIRROR8_MAX_K); 16 = always bf16.
    std::atomic<int64_t> mirror_bits{0};
    std::atomic<uint64_t> st_mirror8_passes{0}, st_mirror8_fallbacks{0}, st_mirror8_unavailable{0}, st_mirror8_breaker_trips{0};
    // Breaker: a corpus the 8-bit certificate cannot settle (tight clusters, duplicates) pays an 8-bit pass plus an f32 scan per query.
    // If kBreakerFails of the last kBreakerWindow 8-bit queries were uncertified, the next kBreakerHold eligible queries take bf16;
    // then the window starts again. (breaker_mu)
    std::mutex breaker_mu;
    uint32_t breaker_bits = 0;           // one bit per collected 8-bit query, newest in bit 0: 1 = uncertified
    int64_t breaker_hold = 0;            // eligible queries still to send to bf16
    // wax_hip_search_batch_submit_device tickets
    struct BatchTicket {
        BatchCtx* c = nullptr;           // null: the batch was answered at submit time (empty engine / loop path)
        const float* d_queries = nullptr;
        wax_hip_hit* d_out = nullptr;
        uint32_t nq = 0, out_stride = 0;
        int k_eff = 0;
        std::thread::id owner;
    };
    std::mutex gemm_chain_mu;                     // "time_kernels": filtering GEMMs of concurrent batches run one after another
    hipEvent_t gemm_chain_ev = nullptr;           // the last one's end-of-kernel event (owned by its workspace)
    TicketTable<BatchTicket> btickets;
    WorkPool<FilterWork> filter_works{4};         // pool of filtered-search workspaces
    IdHash idhash;
    // The per-row columns (DESIGN 2): timestamps and flags (wax_hip_set_attributes), parents (wax_hip_set_parents; DESIGN 4.10), term sets
    // (wax_hip_set_terms; DESIGN 4.11), the group slots derived from the parents, and the marks of their device copies. Everything about
    // them that lives in host memory is in row_columns.h; writers change it under the exclusive engine lock.
    RowColumns cols;
    // How far the bf16 mirror, the code mirror and the id table (`batch`, `idhash`) have followed the store: derived_rows.h. One call per
    // mutation, under the exclusive engine lock.
    DerivedRows derived;
    // Device copy of the attributes, [attr_cap] of each: the first predicate search after a change uploads from cols.attr_mark() on its
    // workspace stream (ensure_attrs, api_predicate.inc, under attr_mu and the shared engine lock).
    std::mutex attr_mu;
    int64_t* d_attr_ts = nullptr;
    uint32_t* d_attr_flags = nullptr;
    uint64_t attr_cap = 0;
    std::atomic<uint64_t> st_attr_uploaded{0};
    // Device copy of the group slots (ensure_groups, api_grouped.inc, under grp_mu and the shared engine lock): the slot of every row and
    // the root id of every slot. Neither exists while the store has no parents.
    std::mutex grp_mu;
    uint32_t* d_grp_slot = nullptr;               // [grp_cap]
    uint64_t* d_grp_root = nullptr;               // [grp_root_cap], the first grp_root_dev entries uploaded under numbering grp_root_epoch
    uint64_t grp_cap = 0, grp_root_cap = 0, grp_root_dev = 0, grp_root_epoch = 0;
    // wax_hip_group_stats (a read-out, no tuning key)
    std::atomic<uint64_t> gs_searches{0}, gs_fused_scans{0}, gs_column_scans{0}, gs_member_rounds{0}, gs_group_slots{0}, gs_parent_rows_uploaded{0};
    // Device copy of the term CSR (ensure_terms, api_terms.inc, under term_mu and the shared engine lock): d_term_off[term_off_cap] holds
    // count + 1 offsets, d_term_val[term_val_cap] the values (the capacity a multiple of 4 words: term_mask_kernel reads whole dwordx4).
    std::mutex term_mu;
    uint32_t* d_term_off = nullptr;
    uint32_t* d_term_val = nullptr;
    uint64_t term_off_cap = 0, term_val_cap = 0;
    // wax_hip_term_stats (a read-out, no tuning key)
    std::atomic<uint64_t> tm_searches{0}, tm_device_masks{0}, tm_host_staged{0}, tm_host_decided{0}, tm_rows_uploaded{0}, tm_values_uploaded{0};
    // wax_hip_term_batch_stats (a read-out of its own)
    std::atomic<uint64_t> tb_calls{0}, tb_queries{0}, tb_sets{0}, tb_mask_launches{0}, tb_looped{0}, tb_host_decided{0};
    std::atomic<int64_t> predicate_route{0};     // 0 = auto, 1 = always gather the passing rows, 2 = the masked scan wherever it is eligible
    // auto rule: the masked scan when at least this many rows per thousand pass. 500 = the random mask's crossover of the FIRST build
    // (between 1/8 and 1/2 passing, profiles/r13/c_routes_first_build.json). At 10M rows the committed f32 scan crosses the gather
    // between 1/2 and 15/16, its mirror form between 1/8 and 1/2 (profiles/r20/predicate_mirror.json; DESIGN 4.5): not retuned.
    std::atomic<int64_t> predicate_scan_min_permille{500};
    std::atomic<uint64_t> st_predicate_searches{0}, st_predicate_gather{0}, st_predicate_masked{0}, st_predicate_skipped{0};
    // the masked scan over the bf16 mirror + f32 re-score + certificate (DESIGN 4.5): 1 (default) = stores of > SCAN_KWAY_MAX_BYTES of
    // rows while "scan_mirror" != 0, 2 = every store, 0 = never
    std::atomic<int64_t> predicate_mirror{1};
    std::atomic<uint64_t> st_predicate_mirror_scans{0}, st_predicate_mirror_fallbacks{0}, st_predicate_mirror_unavailable{0};
    // Predicate tickets (wax_hip_search_predicate_submit; DESIGN 4.5): the bitmap entries (pred_mu) and the counters of
    // wax_hip_predicate_ticket_stats. A sharded handle keeps its own pt_submitted / pt_deferred here and nothing else.
    std::mutex pred_mu;
    PredEntry pred_entries[kPredEntries];
    uint64_t pred_tick = 0;
    std::atomic<uint64_t> pt_submitted{0}, pt_rode{0}, pt_masked_passes{0}, pt_certified{0}, pt_fallbacks{0}, pt_deferred{0}, pt_host_decided{0},
        pt_bitmap_builds{0}, pt_bitmap_hits{0};
    std::atomic<int64_t> filter_device_min{4096}; // allow-lists at least this long are resolved on the device
    std::atomic<uint64_t> st_filter_device{0};    // filtered searches whose allow-list was resolved on the device
    std::atomic<int64_t> filter_batch{1};         // wax_hip_search_batch_filtered: 1 = one gather pass for all lists, 0 = the per-query loop
    std::atomic<uint64_t> st_filter_batch_queries{0}, st_filter_batch_fallbacks{0};
    // wax_hip_search_batch_predicate: row slots one call may spend on entries with a predicate (an entry without a list costs `count`
    // whatever passes). 2^26 slots = 256 MB of row indices: a memory cap, not a tuned number.
    std::atomic<int64_t> predicate_batch_rows{1ll << 26};
    std::atomic<uint64_t> st_predicate_batch_queries{0}, st_predicate_batch_classes{0};   // predicates the batched pass answered / entries with one it built
    // wax_hip_search_many (DESIGN 4.8): 1 = this engine's pairs may share the pooled launch, 0 = each takes the single-query search;
    // stores above search_many_max_rows rows always do. 262 144 = the first power of two above the vec segment cap at 384-d
    // (a placeholder until tools/search_many_bench.py has been run: DESIGN 4.8).
    std::atomic<int64_t> search_many{1};
    std::atomic<int64_t> search_many_max_rows{262144};
    std::atomic<uint64_t> st_many_pooled{0}, st_many_looped{0};   // pairs of this engine answered by the pooled launch / by the single-query search
    std::atomic<uint64_t> st_many_masked{0};                      // ... of the pooled ones, by a group that read a row bitmap (wax_hip_search_many_predicate)
    // Write-combining of single-frame appends (the reference appends into a unified-memory buffer and the GPU simply
    // sees it, MetalVectorEngine.swift:340-351; with discrete HBM the analogue is a pinned staging area that the NEXT
    // reader — or a full staging area — uploads in one copy). The last `pend_rows` rows of [0, count) live only here.
    float* h_pend = nullptr;                 // pinned, pend_cap rows x dims
    uint64_t pend_cap = 0;
    std::atomic<uint64_t> pend_rows{0};
    std::mutex pend_mu;

    // stats
    std::atomic<uint64_t> st_searches{0}, st_rows{0}, st_bytes{0}, st_alloc{0}, st_reuse{0};
    std::mutex st_mu;
    double st_last_ms = 0.0, st_total_ms = 0.0;
    uint64_t st_timed = 0;
    double st_gemm_ms = 0.0;
    uint64_t st_gemm_timed = 0, st_gemm_rows = 0, st_gemm_queries = 0;
};

namespace {

constexpr uint64_t kBounceBytes = 64ull << 20;

// The same for wax_hip_timeline_device, which reads the id table and the attribute columns on its caller's stream: waited for by
// every writer, wax_hip_set_attributes included (the next upload of the columns overwrites what such a launch reads).
void sync_timeline_work(wax_hip_engine* e) {
    for (auto& t : e->tl_ring) {
        std::unique_lock<std::mutex> g(t.mu);
        if (t.busy) {
            (void)hipEventSynchronize(t.done);
            t.busy = false;
        }
    }
}

// Wait until no shard-path work (wax_hip_search_shard_device: enqueued on caller streams, not synchronised by the
// call) is in flight. Called by writers under the exclusive lock, so no new shard work can start meanwhile.
void sync_shard_work(wax_hip_engine* e) {
    for (int r = 0; r < kShardRing; ++r) {
        std::unique_lock<std::mutex> g(e->ring_mu[r]);
        if (e->ring_busy[r]) {
            (void)hipEventSynchronize(e->ring_done[r]);
            e->ring_busy[r] = false;
        }
    }
    sync_timeline_work(e);
}

int holding(wax_hip_engine* e) { return e->holders.holding(); }   // uncollected tickets submitted by the calling thread
// The read side of WriteGuard: the shared lock for the scope, re-entrant for a thread that holds uncollected tickets (RWLock::lock_shared).
struct ReadGuard {
    RWLock& l;
    const bool holder;   // the calling thread holds tickets of this engine
    explicit ReadGuard(wax_hip_engine* e) : l(e->lock), holder(holding(e) > 0) { l.lock_shared(holder); }
    ~ReadGuard() { l.unlock_shared(); }
};

// sharded.inc (included at the end of this file)
int sh_add_batch(wax_hip_engine* e, const uint64_t* frame_ids, const float* rows, uint64_t n, uint32_t dims);
int sh_add_batch_device(wax_hip_engine* e, const uint64_t* frame_ids, const float* d_rows, uint64_t n, uint32_t dims);
int sh_remove(wax_hip_engine* e, uint64_t frame_id);
int sh_remove_batch(wax_hip_engine* e, const uint64_t* frame_ids, uint64_t n, uint64_t* out_removed);
int sh_reserve(wax_hip_engine* e, uint64_t rows);
// What wax_hip_search_predicate_submit adds to a ticket: the score cut its collect applies and, if not null, its row predicate —
// normalised and not empty (DESIGN 4.5, "Predicate tickets").
struct TicketExtras {
    int has_cut;
    float cut;
    const wax_hip_row_predicate* pred;
};
int sh_submit(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, uint64_t* out_ticket, const TicketExtras* x = nullptr);
int sh_collect(wax_hip_engine* e, uint64_t ticket, uint64_t* out_ids, float* out_scores, uint32_t capacity, uint32_t* out_count);
int sh_search_batch_hits(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k, wax_hip_hit* out_hits,
                         uint32_t stride, uint32_t* out_counts);
int sh_batch_device(wax_hip_engine* e, const float* d_queries, uint32_t nq, uint32_t dims, int32_t top_k, wax_hip_hit* d_out_hits,
                    uint32_t out_stride, void* stream, uint64_t* ticket);
int sh_batch_collect_device(wax_hip_engine* e, uint64_t ticket, uint32_t* out_fallbacks);
int sh_search_batch_predicate(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k, const uint64_t* allow,
                              uint64_t n_allow_ids, const uint64_t* allow_begin, const uint64_t* allow_len, const float* min_scores,
                              const wax_hip_row_predicate* preds, uint64_t* out_ids, float* out_scores, uint32_t out_stride, uint32_t* out_counts,
                              const uint32_t* required_terms = nullptr, uint64_t n_required_terms = 0, const uint64_t* term_begin = nullptr,
                              const uint32_t* term_len = nullptr);
int sh_search_filtered(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, int has_allow, const uint64_t* allow,
                       uint64_t n_allow, int has_min, float min_score, uint64_t* out_ids, float* out_scores, uint32_t capacity,
                       uint32_t* out_count);
int sh_set_attributes(wax_hip_engine* e, const uint64_t* frame_ids, const int64_t* timestamps, const uint32_t* flags, uint64_t n,
                      uint64_t* out_applied);
int sh_get_attributes(wax_hip_engine* e, const uint64_t* frame_ids, uint64_t n, int64_t* out_ts, uint32_t* out_flags, uint8_t* out_found);
int sh_search_predicate(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, int has_allow, const uint64_t* allow,
                        uint64_t n_allow, int has_min, float min_score, const wax_hip_row_predicate* pred, uint64_t* out_ids,
                        float* out_scores, uint32_t capacity, uint32_t* out_count, bool caller_locked = false);
int sh_timeline(wax_hip_engine* e, int32_t limit, int newest_first, const wax_hip_row_predicate* pred, uint64_t* out_ids, int64_t* out_ts,
                uint32_t capacity, uint32_t* out_count);
int sh_set_parents(wax_hip_engine* e, const uint64_t* frame_ids, const uint64_t* parent_ids, uint64_t n, uint64_t* out_applied);
int sh_get_parents(wax_hip_engine* e, const uint64_t* frame_ids, uint64_t n, uint64_t* out_parents, uint8_t* out_found);
int sh_search_grouped(wax_hip_engine* e, const float* query, uint32_t dims, int32_t limit, int32_t per_group, int has_min_score, float min_score,
                      const wax_hip_row_predicate* pred, uint64_t* out_root_ids, float* out_root_scores, uint64_t* out_member_ids,
                      float* out_member_scores, uint32_t* out_member_counts, uint32_t* out_count);
int sh_group_stats(wax_hip_engine* e, wax_hip_group_stats_t* out);
int sh_set_terms(wax_hip_engine* e, const uint64_t* frame_ids, uint64_t n, const TermPlan& plan, uint64_t* out_applied);
int sh_get_terms(wax_hip_engine* e, uint64_t frame_id, uint32_t* out_terms, uint32_t out_capacity, uint32_t* out_count, uint8_t* out_found);
int sh_search_terms(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, int has_allow, const uint64_t* allow, uint64_t n_allow,
                    int has_min, float min_score, const wax_hip_row_predicate* pred, const uint32_t* required, uint32_t n_required,
                    uint64_t* out_ids, float* out_scores, uint32_t capacity, uint32_t* out_count);
int sh_term_stats(wax_hip_engine* e, wax_hip_term_stats_t* out);
int sh_term_batch_stats(wax_hip_engine* e, wax_hip_term_batch_stats_t* out);
int sh_serialize(wax_hip_engine* e, uint8_t** out_bytes, size_t* out_len);
int sh_deserialize(wax_hip_engine* e, const uint8_t* data, size_t len);
void sh_destroy(wax_hip_engine* e);
uint64_t sh_total_count(const wax_hip_engine* e);
int sh_stats(wax_hip_engine* e, wax_hip_stats_t* out);
int sh_set_tuning(wax_hip_engine* e, const std::string& k, int64_t value);
int64_t sh_get_tuning(wax_hip_engine* e, const std::string& k);
#define SHARDED_UNSUPPORTED(e, what)                                                                                 \
    do {                                                                                                             \
        if ((e) && (e)->sh) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, what " is a single-device entry point: not available on a sharded engine"); \
    } while (0)
// Mutating entry points: a thread holding uncollected tickets holds the shared lock and would wait for itself.
#define REFUSE_IF_HOLDING(e)                                                                                        \
    do {                                                                                                            \
        if (holding(e) > 0)                                                                                         \
            return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "collect outstanding search tickets first (a ticket holds the engine's read lock)"); \
    } while (0)

