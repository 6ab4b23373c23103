// sharded.inc — the multi-GPU engine behind the same C ABI (SURVEY.md §8b / §8e): one wax_hip_engine handle that owns
// one single-device engine ("shard") per listed device. Included by engine.hip (same translation unit: it uses the
// single-device engine's internals directly).
//
// The reference has no multi-device path (SURVEY.md §2b); what must be preserved is the CONTRACT of
// VectorSearchEngine (VectorSearchEngine.swift:10-18) on top of it: the same results as ONE engine holding all the rows,
// including the tie rule (distance asc, row asc) and the row order `serialize` writes.
//
//   * Layout: contiguous row blocks. Shard g holds global rows [base_g, base_g + count_g) with base_g = the sum of the
//     counts before it, so the concatenation of the shards IS the global row order (= insertion order, as in
//     MetalVectorEngine: append at the end, order-preserving remove, :330-444). New rows go to the last non-full shard;
//     a shard is full at `block_rows` rows (set by reserve(N) to ceil(N / G), or by the first batch, and doubled — with a
//     peer-copy rebalance — when every shard is full). remove() is local to one shard plus G scalar base updates.
//   * Keys carry base_g + local row (wax_hip_set_row_base's mechanism), so every shard's hits are already in the global
//     order and a merge by key gives bit-identical results at any shard count.
//   * search: the host enqueues, per shard and on that shard's own stream, query upload + fused scan + per-shard
//     top-k (wax_hip_search_shard_device) + a peer copy of the k hits (16 k bytes) into device 0's gather buffer;
//     device 0 waits for the G events and merges G k -> k (merge_hits_kernel) into pinned memory. No host round trip
//     between the scan and the merge; nothing but k hits crosses xGMI. "exchange" = 1 swaps the peer copies for one
//     ncclAllGather per query on a single-process communicator (ncclCommInitAll), librccl loaded with dlopen.
//   * batched search: every shard answers the whole batch on its rows (bf16 MFMA path, device-resident entry point)
//     from its own host thread; device 0 merges per query (merge_batch_hits).
//   * mutations take the handle's exclusive lock; searches its shared lock — the reader/writer contract of
//     AsyncReadWriteLock (ReadWriteLock.swift:79-156), as for one engine.
//   * what needs no device lives in two host-only headers, tested on the CPU: the layout decisions in shard_layout.h, the host merges of
//     the shards' answers in shard_merge.h. This file carries them out.
#include <dlfcn.h>

#include <functional>

namespace {

constexpr int kShardMaxK = FUSED_MAX_K;     // device-side gather + merge serves k <= 192; larger k merges on the host
constexpr int kShardSlots = 8;              // sharded single-query searches in flight per handle (soft cap: callers without tickets wait)
constexpr int kShardHardSlots = 64;         // hard cap for a thread that pipelines submits without collecting

struct RcclApi {
    void* lib = nullptr;
    int (*CommInitAll)(void** comms, int ndev, const int* devlist) = nullptr;
    int (*CommDestroy)(void* comm) = nullptr;
    int (*CommCount)(void* comm, int* count) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*AllGather)(const void* send, void* recv, size_t count, int datatype, void* comm, hipStream_t stream) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};

struct ShardSlot {
    std::vector<wax_hip_hit*> d_hits;       // per shard, on its device: [kShardMaxK] (rccl: [G][kShardMaxK] gathered)
    std::vector<wax_hip_hit*> d_send;       // rccl exchange only: per shard send buffer [kShardMaxK]
    wax_hip_hit* d_gather = nullptr;        // device of shard 0: [G][kShardMaxK]
    wax_hip_hit* d_merged = nullptr;        // device of shard 0: [kShardMaxK]
    wax_hip_hit* h_out = nullptr;           // pinned [kShardMaxK]
    std::vector<hipEvent_t> ev;             // per shard: its part is in the gather buffer
    hipEvent_t done = nullptr;
    // ticket state
    std::thread::id owner;                  // submitting thread (ticket ownership, as for one engine)
    int kpad = 0;                           // hits per shard on the device path (0 = host path or empty)
    bool host_path = false;
    std::vector<uint64_t> sub_tickets;      // ticket path: one ticket per shard that holds rows (0 = none)
    int only_shard = -1;                    // ticket path with ONE shard holding rows: collect goes straight to that engine
    int32_t top_k = 0;
    // wax_hip_search_predicate_submit on a handle: the score cut of the ticket, and a ticket with a predicate — always deferred: its
    // collect runs sh_search_predicate under the lock the ticket holds
    bool has_cut = false;
    float cut = 0.f;
    bool pred_deferred = false;
    wax_hip_row_predicate pred{};
    std::vector<float> query;
};

// Workspace of one batched search on a sharded handle (pooled; nothing is allocated per call once warm).
struct ShardBatchWork {
    std::vector<float*> d_q;                // per shard, on its device: the query block (unused where the shard shares the caller's device)
    std::vector<uint64_t> q_cap;            // in floats
    std::vector<wax_hip_hit*> d_part;       // per shard, on its device: [nq][k] its hits
    std::vector<uint64_t> part_cap;         // in hits
    wax_hip_hit* d_all = nullptr;           // first device: [G][nq][k] gathered
    uint64_t all_cap = 0;
    std::vector<hipEvent_t> ev;             // per shard: its part is in d_all
    hipEvent_t ev_in = nullptr;             // first device: the caller's stream has produced the queries
    hipEvent_t done = nullptr;
    // host-pointer calls
    float* d_q0 = nullptr; uint64_t q0_cap = 0;           // first device: uploaded queries
    wax_hip_hit* d_out0 = nullptr; uint64_t out0_cap = 0; // first device: merged hits
    wax_hip_hit* h_out = nullptr; uint64_t hout_cap = 0;  // pinned
    // ticket state
    std::vector<uint64_t> sub_tickets;
    std::vector<uint8_t> sub_valid;
    const float* d_queries = nullptr;
    wax_hip_hit* d_out = nullptr;
    uint32_t nq = 0, k = 0, out_stride = 0;
    std::thread::id owner;
};

struct ShardedState {
    std::vector<wax_hip_engine*> subs;
    std::vector<int> devices;
    std::vector<hipStream_t> streams;       // one per shard, on its device
    hipStream_t merge_stream = nullptr;     // device of shard 0
    ShardLayout layout;                     // block_rows, reserve_hint and every decision that follows from the shards' counts (shard_layout.h)
    WorkPool<ShardSlot> slots{kShardSlots, kShardHardSlots};
    TicketTable<ShardSlot*> tickets;
    std::atomic<int64_t> exchange{0};       // 0 = peer copies (default), 1 = RCCL all-gather
    RcclApi rccl;
    std::vector<void*> comms;
    std::mutex rccl_mu;                     // one ncclGroupStart .. ncclGroupEnd section at a time (concurrent submitters share the communicators)
    std::atomic<uint64_t> rccl_collectives{0};
    // Peer access between the first device (gather / merge / query source) and every other shard's device, both directions.
    // peer_pairs = pairs that need it, peer_enabled = pairs where hipDeviceCanAccessPeer said yes and the enable went through.
    // When a pair lacks it the k-hit gather does not rely on the runtime's implicit staging: single-query searches take the
    // host path (per-shard tickets, D2H of k hits each, host merge by key — the code k > 192 always uses).
    int peer_pairs = 0, peer_enabled = 0;
    bool host_gather = false;               // forced host-side gather + merge (no peer access, or "gather" = 2)
    // Single-query searches (round 5). 1 (default) = per-shard tickets: every shard that holds rows answers through its own
    // engine's one-launch path (query in the kernel arguments, k-way merge in the scan kernel, hits + completion word straight
    // into pinned memory), submitted side by side by the persistent workers, merged by key on the host at collect (G x k keys).
    // 0 = the round-2 device gather (per shard: upload, scan, merge, peer copy, event; then a merge launch on the first device):
    // still what "exchange" = 1 (RCCL) uses.
    std::atomic<int64_t> ticket_path{1};
    std::atomic<uint64_t> ticket_searches{0}, single_shard_searches{0}, inline_fanouts{0};
    // Small-store rule: a shard's block is at least this many MB of rows, so a store below it lives on the FIRST device only
    // (a 15 MB store spread over 8 GPUs is 8 launches and a gather for 2 MB of scan each). 0 = spread from the first row.
    std::atomic<int64_t> shard_min_mb{64};
    std::atomic<uint64_t> rebalances{0};
    ShardWorkers workers;
    WorkPool<ShardBatchWork> bworks{4};
    TicketTable<ShardBatchWork*> btickets;
    // batched collect: the shards' collects run one after the other on the calling thread (each is just a wait when every
    // query was certified on the device) — unless the previous batch had two or more shards settle queries on the host side
    // (full retries / exact passes: data with dense neighbourhoods, which tends to persist from batch to batch); then the
    // per-shard collects go to the persistent workers and those ladders run side by side.
    std::atomic<int> collect_parallel{0};
    std::atomic<uint64_t> parallel_collects{0};
    std::atomic<uint64_t> parallel_submits{0};      // batches whose per-shard submits ran on the workers (a submit would have blocked)
};

uint64_t sh_count(const ShardedState* s) {
    uint64_t n = 0;
    for (auto* e : s->subs) n += e->count;
    return n;
}

// what the layout decides from
std::vector<uint64_t> sh_counts(const ShardedState* s) {
    std::vector<uint64_t> counts;
    for (auto* e : s->subs) counts.push_back(e->count);
    return counts;
}

ShardLayout::Shape sh_shape(const ShardedState* s, uint32_t dims) {
    return ShardLayout::Shape{s->subs.size(), dims, s->shard_min_mb.load(), WAX_HIP_INITIAL_RESERVE};
}

void sh_update_bases(ShardedState* s) {
    const std::vector<uint64_t> bases = ShardLayout::bases(sh_counts(s).data(), s->subs.size());
    for (size_t g = 0; g < bases.size(); ++g) s->subs[g]->row_base = bases[g];   // under the handle's exclusive lock: no shard search is in flight
}

// (shard, local row) of a frame id, or shard = -1
int sh_find(ShardedState* s, uint64_t id, int64_t* local) {
    for (size_t g = 0; g < s->subs.size(); ++g) {
        const int64_t r = s->subs[g]->idmap.find(id);
        if (r >= 0) { *local = r; return (int)g; }
    }
    return -1;
}

// The ids of a call by owning shard: per shard the caller positions it owns and their local rows, call order kept inside a shard (so the
// last entry of a repeated id still wins). Absent ids are in no shard's list. Callers gather their own payload columns through `at`.
struct ShardRoute {
    std::vector<uint64_t> at;       // positions in the caller's arrays
    std::vector<uint64_t> ids;      // frame_ids[at[j]]
    std::vector<uint64_t> rows;     // local row of ids[j]
    template <typename T>
    std::vector<T> gather(const T* column) const {       // (a null column: nothing)
        std::vector<T> out;
        for (size_t j = 0; column && j < at.size(); ++j) out.push_back(column[at[j]]);
        return out;
    }
};
std::vector<ShardRoute> sh_route(ShardedState* s, const uint64_t* frame_ids, uint64_t n) {
    std::vector<ShardRoute> routes(s->subs.size());
    for (uint64_t i = 0; i < n; ++i) {
        int64_t local = -1;
        const int g = sh_find(s, frame_ids[i], &local);
        if (g < 0) continue;
        routes[(size_t)g].at.push_back(i);
        routes[(size_t)g].ids.push_back(frame_ids[i]);
        routes[(size_t)g].rows.push_back((uint64_t)local);
    }
    return routes;
}

int sh_load_rccl(ShardedState* s) {
    if (s->rccl.lib) return WAX_HIP_OK;
    void* lib = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);          // the copy the process already uses (e.g. torch's), if any
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!lib) return fail(WAX_HIP_ERR_INTERNAL, std::string("RCCL exchange requested but librccl could not be loaded: ") + dlerror());
    RcclApi& r = s->rccl;
    r.CommInitAll = reinterpret_cast<decltype(r.CommInitAll)>(dlsym(lib, "ncclCommInitAll"));
    r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
    r.CommCount = reinterpret_cast<decltype(r.CommCount)>(dlsym(lib, "ncclCommCount"));
    r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(dlsym(lib, "ncclGroupStart"));
    r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(dlsym(lib, "ncclGroupEnd"));
    r.AllGather = reinterpret_cast<decltype(r.AllGather)>(dlsym(lib, "ncclAllGather"));
    r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
    if (!r.CommInitAll || !r.CommDestroy || !r.GroupStart || !r.GroupEnd || !r.AllGather)
        return fail(WAX_HIP_ERR_INTERNAL, "librccl lacks the ncclCommInitAll / ncclAllGather entry points");
    s->comms.assign(s->subs.size(), nullptr);
    const int rc = r.CommInitAll(s->comms.data(), (int)s->devices.size(), s->devices.data());
    if (rc != 0) {
        s->comms.clear();
        return fail(WAX_HIP_ERR_INTERNAL, std::string("ncclCommInitAll failed: ") + (r.GetErrorString ? r.GetErrorString(rc) : "?") +
                                              " (RCCL needs distinct devices)");
    }
    r.lib = lib;
    return WAX_HIP_OK;
}

void sh_free_slot(ShardedState* s, ShardSlot* sl) {
    if (!sl) return;
    for (size_t g = 0; g < sl->d_hits.size(); ++g) {
        DeviceGuard dg(s->devices[g]);
        (void)hipFree(sl->d_hits[g]);
        if (g < sl->d_send.size()) (void)hipFree(sl->d_send[g]);
        if (g < sl->ev.size() && sl->ev[g]) (void)hipEventDestroy(sl->ev[g]);
    }
    {
        DeviceGuard dg(s->devices[0]);
        (void)hipFree(sl->d_gather); (void)hipFree(sl->d_merged); (void)hipHostFree(sl->h_out);
        if (sl->done) (void)hipEventDestroy(sl->done);
    }
    delete sl;
}

int sh_alloc_slot(ShardedState* s, ShardSlot** out) {
    const size_t G = s->subs.size();
    ShardSlot* sl = new ShardSlot();
    sl->d_hits.assign(G, nullptr); sl->d_send.assign(G, nullptr); sl->ev.assign(G, nullptr);
    hipError_t err = hipSuccess;
    for (size_t g = 0; g < G && err == hipSuccess; ++g) {
        DeviceGuard dg(s->devices[g]);
        err = hipMalloc(&sl->d_hits[g], (size_t)G * kShardMaxK * sizeof(wax_hip_hit));   // [G][k]: also the all-gather receive buffer
        if (err == hipSuccess) err = hipMalloc(&sl->d_send[g], (size_t)kShardMaxK * sizeof(wax_hip_hit));
        if (err == hipSuccess) err = hipEventCreateWithFlags(&sl->ev[g], hipEventDisableTiming);
    }
    if (err == hipSuccess) {
        DeviceGuard dg(s->devices[0]);
        err = hipMalloc(&sl->d_gather, (size_t)G * kShardMaxK * sizeof(wax_hip_hit));
        if (err == hipSuccess) err = hipMalloc(&sl->d_merged, (size_t)kShardMaxK * sizeof(wax_hip_hit));
        if (err == hipSuccess) err = hipHostMalloc(&sl->h_out, (size_t)kShardMaxK * sizeof(wax_hip_hit), hipHostMallocDefault);
        if (err == hipSuccess) err = hipEventCreateWithFlags(&sl->done, hipEventDisableTiming);
    }
    if (err != hipSuccess) {
        sh_free_slot(s, sl);
        return fail(WAX_HIP_ERR_ALLOC, std::string("Failed to allocate sharded search scratch: ") + hipGetErrorString(err));
    }
    *out = sl;
    return WAX_HIP_OK;
}

// `holder`: the calling thread already owns tickets of this handle (= slots, and the shared lock), so like take_slot's it never
// WAITS for a slot (work_pool.h, PoolMode::grow): a freshly allocated one beyond kShardSlots, up to kShardHardSlots, and an error
// after that. Returned by s->slots.release(sl).
int sh_take_slot(ShardedState* s, ShardSlot** out, bool holder) {
    int rc = WAX_HIP_OK;
    const PoolGot got = s->slots.acquire(holder ? PoolMode::grow : PoolMode::wait, out, &rc, [s](int, ShardSlot** made) { return sh_alloc_slot(s, made); });
    return got == PoolGot::exhausted ? fail(WAX_HIP_ERR_INVALID_ARGUMENT, "too many outstanding search tickets (collect some first)") : rc;
}

// per_shard(g) -> rc on every shard; the lowest failing shard's code and text (a worker's g_last_error is its own thread's) become the
// caller's through fail().
enum class FanOut {
    workers,           // side by side on the persistent workers (each bound to its shard's device); one shard: the caller's thread
    workers_if_free,   // the same unless another job holds the workers: then the caller's thread at once, and *ran_inline says so
    serial_stop,       // the caller's thread, shard after shard, stopping at the first failure
    serial_all,        // the caller's thread, every shard whatever the others returned
};
template <typename PerShard>
int sh_fan_out(ShardedState* s, FanOut mode, PerShard per_shard, bool* ran_inline = nullptr) {
    const size_t G = s->subs.size();
    std::vector<int> rcs(G, WAX_HIP_OK);
    std::vector<std::string> errs(G);
    const std::function<void(size_t)> one = [&](size_t g) {
        rcs[g] = per_shard(g);
        if (rcs[g] != WAX_HIP_OK) errs[g] = g_last_error;
    };
    bool on_workers = false;
    if (mode == FanOut::workers && G > 1) { s->workers.run_all(one); on_workers = true; }
    else if (mode == FanOut::workers_if_free) on_workers = s->workers.try_run_all(one);
    if (ran_inline) *ran_inline = !on_workers;
    if (!on_workers)
        for (size_t g = 0; g < G; ++g) {
            one(g);
            if (rcs[g] != WAX_HIP_OK && mode == FanOut::serial_stop) break;
        }
    for (size_t g = 0; g < G; ++g)
        if (rcs[g] != WAX_HIP_OK) return fail(rcs[g], errs[g]);
    return WAX_HIP_OK;
}

// ---- mutations (handle's exclusive lock held) ---------------------------------------------------------------------

// Move every row of shard `from` to the end of shard `to` (same or another device), in chunks through a buffer on
// `to`'s device; `from` is left empty.
int sh_move_all(ShardedState* s, size_t from, size_t to) {
    wax_hip_engine* src = s->subs[from];
    wax_hip_engine* dst = s->subs[to];
    { const int frc = flush_pending(src); if (frc != WAX_HIP_OK) return frc; }
    const uint64_t n = src->count;
    if (n == 0) return WAX_HIP_OK;
    if (!dst->cols.can_take(src->cols))
        return fail(WAX_HIP_ERR_CAPACITY, "rebalance: the target shard would hold 2^32 terms or more");   // (before any row moves)
    const uint32_t D = src->dims;
    const uint64_t chunk = std::max<uint64_t>(1, (64ull << 20) / ((uint64_t)D * 4));
    float* d_tmp = nullptr;
    {
        DeviceGuard dg(s->devices[to]);
        HIP_TRY(hipMalloc(&d_tmp, (size_t)std::min(chunk, n) * D * sizeof(float)), WAX_HIP_ERR_ALLOC, "Failed to allocate rebalance buffer");
    }
    int rc = WAX_HIP_OK;
    const uint64_t dst_before = dst->count;
    for (uint64_t lo = 0; lo < n && rc == WAX_HIP_OK; lo += chunk) {
        const uint64_t m = std::min(chunk, n - lo);
        hipError_t err = hipMemcpyPeer(d_tmp, s->devices[to], src->d_store + lo * D, s->devices[from], (size_t)m * D * sizeof(float));
        if (err != hipSuccess) { rc = fail(WAX_HIP_ERR_INTERNAL, std::string("rebalance peer copy: ") + hipGetErrorString(err)); break; }
        rc = wax_hip_add_batch_device(dst, src->ids.data() + lo, d_tmp, m, D);
    }
    {
        DeviceGuard dg(s->devices[to]);
        (void)hipFree(d_tmp);
    }
    if (rc != WAX_HIP_OK) {
        // failure-atomic: the chunks already appended to `dst` are taken back (the source still holds every row), so no
        // frame id ever exists in two shards
        for (uint64_t r = dst_before; r < dst->count; ++r) dst->idmap.erase_only(dst->ids[(size_t)r]);
        dst->ids.resize((size_t)dst_before);
        dst->count = dst_before;
        dst->cols.truncate(dst_before);
        dst->derived.replaced();    // (rows were appended and taken back: the mirror and the id table start over)
        return rc;
    }
    // the rows' attributes, parents and term sets travel with them: dst's columns are padded to where the moved rows begin, then take
    // src's, which is left without columns
    dst->cols.take_all(src->cols, dst_before);
    // empty the source (capacity stays)
    src->count = 0;
    src->ids.clear();
    src->idmap.clear();
    src->pend_rows.store(0);
    src->derived.replaced();
    return WAX_HIP_OK;
}

// The shard that takes the next appended row (and how many it can take). When all are full the layout doubles its blocks
// (ShardLayout::doubling_moves: in place, in an order that never overwrites a source) and the rows move here.
int sh_next_tail(ShardedState* s, size_t* shard, uint64_t* room) {
    while (!s->layout.tail(sh_counts(s).data(), s->subs.size(), shard, room)) {
        for (const auto& move : ShardLayout::doubling_moves(s->subs.size())) {
            const int rc = sh_move_all(s, move.first, move.second);
            if (rc != WAX_HIP_OK) {
                // A failed move left both shards as they were, but earlier moves of this pass have already happened: the rows are
                // all still there, in global order, yet no longer in blocks of `block_rows`. Bases follow the counts; appends keep
                // working (the tail is found from the counts only).
                sh_update_bases(s);
                return rc;
            }
        }
        s->layout.doubled();
        s->rebalances++;
        sh_update_bases(s);
    }
    return WAX_HIP_OK;
}

int sh_add_batch(wax_hip_engine* e, const uint64_t* frame_ids, const float* rows, uint64_t n, uint32_t dims) {
    ShardedState* s = e->sh;
    if (n == 0) return WAX_HIP_OK;                                        // MetalVectorEngine.swift:360
    if (!frame_ids || !rows) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "addBatch: null input");
    if (dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));   // :367-370
    REFUSE_IF_HOLDING(e);
    WriteGuard w(e->lock);
    if (sh_count(s) + n > 0xffffffffull)
        return fail(WAX_HIP_ERR_CAPACITY, "capacity exceeded: limit 4294967295, requested " + std::to_string(sh_count(s) + n));
    s->layout.first_rows(sh_shape(s, e->dims), n);   // a bulk load spreads evenly, anything else starts from the reserve hint
    // Sequential upsert semantics of MetalVectorEngine.addBatch (:384-398): an id that already exists (anywhere, or
    // earlier in this batch) is overwritten in place; new ids are appended in order. Runs of consecutive new ids go to
    // the tail shard as one batch.
    uint64_t i = 0;
    int rc = WAX_HIP_OK;
    while (i < n && rc == WAX_HIP_OK) {
        int64_t local = -1;
        const int g = sh_find(s, frame_ids[i], &local);
        if (g >= 0) {
            rc = wax_hip_add_batch(s->subs[(size_t)g], frame_ids + i, rows + i * (uint64_t)dims, 1, dims);
            ++i;
            continue;
        }
        size_t tail = 0;
        uint64_t room = 0;
        rc = sh_next_tail(s, &tail, &room);
        if (rc != WAX_HIP_OK) break;
        // extend the run while ids are new (not in any shard, not repeated inside the run) and the shard has room
        IdMap seen;
        uint64_t j = i;
        while (j < n && j - i < room) {
            int64_t l2;
            if (seen.find(frame_ids[j]) >= 0 || sh_find(s, frame_ids[j], &l2) >= 0) break;
            seen.put(frame_ids[j], 0);
            ++j;
        }
        rc = wax_hip_add_batch(s->subs[tail], frame_ids + i, rows + i * (uint64_t)dims, j - i, dims);
        i = j;
    }
    sh_update_bases(s);
    return rc;
}

// Append-only batch whose rows already live in HBM (on any visible device): runs go to the tail shard directly when the
// rows are on its device, through a peer copy otherwise.
int sh_add_batch_device(wax_hip_engine* e, const uint64_t* frame_ids, const float* d_rows, uint64_t n, uint32_t dims) {
    ShardedState* s = e->sh;
    if (n == 0) return WAX_HIP_OK;
    if (!frame_ids || !d_rows) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "addBatch: null input");
    if (dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, d_rows) != hipSuccess) { (void)hipGetLastError(); return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "add_batch_device: not a device pointer"); }
    const int src_dev = attr.device;
    REFUSE_IF_HOLDING(e);
    WriteGuard w(e->lock);
    if (sh_count(s) + n > 0xffffffffull)
        return fail(WAX_HIP_ERR_CAPACITY, "capacity exceeded: limit 4294967295, requested " + std::to_string(sh_count(s) + n));
    IdMap seen;
    for (uint64_t i = 0; i < n; ++i) {
        int64_t l;
        if (seen.find(frame_ids[i]) >= 0 || sh_find(s, frame_ids[i], &l) >= 0)
            return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "add_batch_device: frame id " + std::to_string(frame_ids[i]) + " already present (append-only path)");
        seen.put(frame_ids[i], 0);
    }
    s->layout.first_rows(sh_shape(s, e->dims), n);
    int rc = WAX_HIP_OK;
    uint64_t i = 0;
    float* d_tmp = nullptr;
    int tmp_dev = -1;
    uint64_t tmp_rows = 0;
    while (i < n && rc == WAX_HIP_OK) {
        size_t tail = 0;
        uint64_t room = 0;
        rc = sh_next_tail(s, &tail, &room);
        if (rc != WAX_HIP_OK) break;
        const uint64_t m = std::min(room, n - i);
        const float* src = d_rows + i * (uint64_t)dims;
        if (s->devices[tail] == src_dev) {
            rc = wax_hip_add_batch_device(s->subs[tail], frame_ids + i, src, m, dims);
        } else {
            const uint64_t chunk = std::max<uint64_t>(1, (64ull << 20) / ((uint64_t)dims * 4));
            for (uint64_t lo = 0; lo < m && rc == WAX_HIP_OK; lo += chunk) {
                const uint64_t c = std::min(chunk, m - lo);
                if (tmp_dev != s->devices[tail] || tmp_rows < c) {
                    if (d_tmp) { DeviceGuard dg(tmp_dev); (void)hipFree(d_tmp); d_tmp = nullptr; }
                    DeviceGuard dg(s->devices[tail]);
                    hipError_t err = hipMalloc(&d_tmp, (size_t)std::min(chunk, m) * dims * sizeof(float));
                    if (err != hipSuccess) { rc = fail(WAX_HIP_ERR_ALLOC, std::string("Failed to allocate peer staging: ") + hipGetErrorString(err)); break; }
                    tmp_dev = s->devices[tail]; tmp_rows = std::min(chunk, m);
                }
                hipError_t err = hipMemcpyPeer(d_tmp, s->devices[tail], src + lo * (uint64_t)dims, src_dev, (size_t)c * dims * sizeof(float));
                if (err != hipSuccess) { rc = fail(WAX_HIP_ERR_INTERNAL, std::string("peer copy: ") + hipGetErrorString(err)); break; }
                rc = wax_hip_add_batch_device(s->subs[tail], frame_ids + i + lo, d_tmp, c, dims);
            }
        }
        i += m;
    }
    if (d_tmp) { DeviceGuard dg(tmp_dev); (void)hipFree(d_tmp); }
    sh_update_bases(s);
    return rc;
}

int sh_remove(wax_hip_engine* e, uint64_t frame_id) {
    ShardedState* s = e->sh;
    REFUSE_IF_HOLDING(e);
    WriteGuard w(e->lock);
    int64_t local = -1;
    const int g = sh_find(s, frame_id, &local);
    if (g < 0) return WAX_HIP_OK;                                          // :426 absent id is a no-op
    const int rc = wax_hip_remove(s->subs[(size_t)g], frame_id);           // order-preserving inside the shard (:431-441)
    sh_update_bases(s);
    return rc;
}

// removeBatch on a handle: the ids are grouped by owning shard and every shard that owns any compacts once (one pass over its own
// rows behind its first removed one); the bases follow once at the end. The shards' passes run one after the other.
int sh_remove_batch(wax_hip_engine* e, const uint64_t* frame_ids, uint64_t n, uint64_t* out_removed) {
    ShardedState* s = e->sh;
    if (out_removed) *out_removed = 0;
    if (n == 0) return WAX_HIP_OK;
    if (!frame_ids) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "removeBatch: null input");
    REFUSE_IF_HOLDING(e);
    WriteGuard w(e->lock);
    const std::vector<ShardRoute> per = sh_route(s, frame_ids, n);        // :426 absent ids are ignored
    int rc = WAX_HIP_OK;
    uint64_t total = 0;
    for (size_t g = 0; g < per.size() && rc == WAX_HIP_OK; ++g) {
        if (per[g].ids.empty()) continue;
        uint64_t got = 0;
        rc = wax_hip_remove_batch(s->subs[g], per[g].ids.data(), per[g].ids.size(), &got);
        total += got;
    }
    sh_update_bases(s);
    if (out_removed) *out_removed = total;
    return rc;
}

int sh_reserve(wax_hip_engine* e, uint64_t rows) {
    ShardedState* s = e->sh;
    REFUSE_IF_HOLDING(e);
    WriteGuard w(e->lock);
    if (rows > 0xffffffffull)
        return fail(WAX_HIP_ERR_CAPACITY, "capacity exceeded: limit 4294967295, requested " + std::to_string(rows));
    // an empty engine adopts the layout the caller announced; shards are filled in order: reserve what this many rows will occupy
    // (a store below one block touches the first device only)
    const std::vector<uint64_t> ask = s->layout.reserve(sh_shape(s, e->dims), rows, sh_counts(s).data());
    int rc = WAX_HIP_OK;
    for (size_t g = 0; g < ask.size() && ask[g] > 0 && rc == WAX_HIP_OK; ++g) rc = wax_hip_reserve(s->subs[g], ask[g]);
    return rc;
}

// ---- single-query search ---------------------------------------------------------------------------------------------

int sh_submit(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, uint64_t* out_ticket, const TicketExtras* x) {
    ShardedState* s = e->sh;
    if (!out_ticket) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine/ticket is null");
    e->lock.lock_shared(holding(e) > 0);
    int rc = WAX_HIP_OK;
    ShardSlot* sl = nullptr;
    do {
        const uint64_t total = sh_count(s);
        rc = sh_take_slot(s, &sl, holding(e) > 0);
        if (rc != WAX_HIP_OK) break;
        sl->kpad = 0; sl->host_path = false; sl->top_k = top_k; sl->sub_tickets.clear(); sl->only_shard = -1;
        sl->has_cut = x != nullptr && x->has_cut != 0; sl->cut = x != nullptr ? x->cut : 0.f; sl->pred_deferred = false;
        if (x != nullptr && x->pred != nullptr) e->pt_submitted++;
        if (total == 0) break;                                             // :448 empty engine: an empty ticket
        if (dims != e->dims || !query) { rc = fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, query ? dims : 0)); break; }
        if (x != nullptr && x->pred != nullptr) {                          // no fan-out of predicate tickets: the blocking body at collect
            sl->pred_deferred = true;
            sl->pred = *x->pred;
            sl->query.assign(query, query + dims);
            e->pt_deferred++;
            break;
        }
        const int limit = clamp_topk(top_k);
        const size_t G = s->subs.size();
        const bool rccl_wanted = s->exchange.load() == 1;
        if (limit > kShardMaxK || (s->host_gather && G > 1) || (s->ticket_path.load() != 0 && !rccl_wanted)) {
            // every shard that holds rows answers through its own ticket (one launch per shard on the default path: query in the
            // kernel arguments, merge in the scan kernel, hits and completion word written straight to pinned memory); the host
            // merges by key at collect. Also what large k and devices without peer access have always used.
            sl->host_path = true;
            sl->sub_tickets.assign(G, 0);
            size_t active = 0, last = 0;
            for (size_t g = 0; g < G; ++g)
                if (s->subs[g]->count > 0 || s->subs[g]->pend_rows.load() > 0) { ++active; last = g; }
            if (active <= 1) {
                // small stores live on one device (shard_min_mb): the handle adds a ticket lookup to that engine's own latency
                sl->only_shard = (int)last;
                rc = submit_impl(s->subs[last], query, dims, top_k, &sl->sub_tickets[last], false);
                s->single_shard_searches++;
                break;
            }
            // side by side on the persistent workers (each bound to its shard's device): a fan-out costs one launch time, not G
            // (workers busy with a long job — mirror build, filtered search, k > 192 batch —: G launches from this thread, 3 - 4 us each,
            // instead of waiting milliseconds for the workers; submit_impl binds the shard's device itself)
            bool ran_inline = false;
            rc = sh_fan_out(s, FanOut::workers_if_free, [&](size_t g) {
                wax_hip_engine* sub = s->subs[g];
                if (sub->count == 0 && sub->pend_rows.load() == 0) return (int)WAX_HIP_OK;
                return submit_impl(sub, query, dims, top_k, &sl->sub_tickets[g], false);
            }, &ran_inline);
            if (ran_inline) s->inline_fanouts++;
            s->ticket_searches++;
            break;
        }
        sl->kpad = limit;
        const bool rccl = rccl_wanted;               // also with one shard: a 1-rank communicator (the all-gather is then a copy)
        if (rccl) { rc = sh_load_rccl(s); if (rc != WAX_HIP_OK) break; }
        const float qn = query_norm(query, dims);    // once per query, not once per shard
        for (size_t g = 0; g < G && rc == WAX_HIP_OK; ++g) {
            DeviceGuard dg(s->devices[g]);
            wax_hip_hit* dst = rccl ? sl->d_send[g] : sl->d_hits[g];
            rc = search_shard_device_impl(s->subs[g], query, dims, top_k, dst, s->streams[g], qn);
            if (rc != WAX_HIP_OK) break;
            if (!rccl) {
                hipError_t err = (G == 1) ? hipSuccess
                                          : hipMemcpyPeerAsync(sl->d_gather + g * (size_t)limit, s->devices[0], dst, s->devices[g],
                                                               (size_t)limit * sizeof(wax_hip_hit), s->streams[g]);
                if (err == hipSuccess) err = hipEventRecord(sl->ev[g], s->streams[g]);
                if (err != hipSuccess) rc = fail(WAX_HIP_ERR_INTERNAL, std::string("shard gather: ") + hipGetErrorString(err));
            }
        }
        if (rc != WAX_HIP_OK) break;
        if (rccl) {
            // one all-gather per query on the single-process communicator: every shard ends up with all G k hits
            RcclApi& r = s->rccl;
            std::unique_lock<std::mutex> rg(s->rccl_mu);
            int nrc = r.GroupStart();
            for (size_t g = 0; g < G && nrc == 0; ++g)
                nrc = r.AllGather(sl->d_send[g], sl->d_hits[g], (size_t)limit * 2, /*ncclInt64*/ 4, s->comms[g], s->streams[g]);
            if (nrc == 0) nrc = r.GroupEnd();
            rg.unlock();
            if (nrc != 0) { rc = fail(WAX_HIP_ERR_INTERNAL, std::string("ncclAllGather failed: ") + (r.GetErrorString ? r.GetErrorString(nrc) : "?")); break; }
            s->rccl_collectives++;
            DeviceGuard dg(s->devices[0]);
            hipError_t err = hipEventRecord(sl->ev[0], s->streams[0]);
            if (err != hipSuccess) { rc = fail(WAX_HIP_ERR_INTERNAL, std::string("event record: ") + hipGetErrorString(err)); break; }
        }
        // device of shard 0: wait for every part, merge G k -> k into pinned memory
        DeviceGuard dg(s->devices[0]);
        hipError_t err = hipSuccess;
        for (size_t g = 0; g < (rccl ? 1 : G) && err == hipSuccess; ++g) err = hipStreamWaitEvent(s->merge_stream, sl->ev[g], 0);
        if (err == hipSuccess) {
            if (G == 1) {
                err = hipMemcpyAsync(sl->h_out, sl->d_hits[0], (size_t)limit * sizeof(wax_hip_hit), hipMemcpyDeviceToHost, s->merge_stream);
            } else {
                const wax_hip_hit* src = rccl ? sl->d_hits[0] : sl->d_gather;
                err = launch_merge_hits(src, (uint32_t)(G * (size_t)limit), limit, sl->d_merged, s->merge_stream);
                if (err == hipSuccess)
                    err = hipMemcpyAsync(sl->h_out, sl->d_merged, (size_t)limit * sizeof(wax_hip_hit), hipMemcpyDeviceToHost, s->merge_stream);
            }
        }
        if (err == hipSuccess) err = hipEventRecord(sl->done, s->merge_stream);
        if (err != hipSuccess) rc = fail(WAX_HIP_ERR_INTERNAL, std::string("shard merge: ") + hipGetErrorString(err));
    } while (0);
    if (rc != WAX_HIP_OK) {
        if (sl) {
            std::string keep = g_last_error;
            for (size_t g = 0; g < sl->sub_tickets.size(); ++g)
                if (sl->sub_tickets[g]) { uint32_t dummy = 0; std::vector<wax_hip_hit> tmp(1); (void)collect_impl(s->subs[g], sl->sub_tickets[g], nullptr, nullptr, 0, &dummy, tmp.data(), 0); }
            for (size_t g = 0; g < s->subs.size(); ++g) { DeviceGuard dg(s->devices[g]); (void)hipStreamSynchronize(s->streams[g]); }
            g_last_error = keep;
            s->slots.release(sl);
        }
        e->lock.unlock_shared();
        return rc;
    }
    *out_ticket = s->tickets.put(sl);
    e->holders.note_submit(&sl->owner);   // ticket ownership, as for one engine (the shared lock is held until collect)
    return WAX_HIP_OK;
}

int sh_collect(wax_hip_engine* e, uint64_t ticket, uint64_t* out_ids, float* out_scores, uint32_t capacity, uint32_t* out_count) {
    ShardedState* s = e->sh;
    if (!out_count) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine/out_count is null");
    ShardSlot* sl = nullptr;
    if (!s->tickets.take(ticket, &sl)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "unknown ticket " + std::to_string(ticket));
    int rc = WAX_HIP_OK;
    *out_count = 0;
    if ((!out_ids || !out_scores) && capacity > 0) rc = fail(WAX_HIP_ERR_INVALID_ARGUMENT, "output arrays are null");
    if (sl->pred_deferred) {
        if (rc == WAX_HIP_OK)   // (the cut is the shards' own, as in the blocking call)
            rc = sh_search_predicate(e, sl->query.data(), e->dims, sl->top_k, 0, nullptr, 0, sl->has_cut ? 1 : 0, sl->cut, &sl->pred, out_ids, out_scores,
                                     capacity, out_count, /*caller_locked=*/true);
    } else if (sl->host_path && sl->only_shard >= 0) {
        // one shard holds every row: its keys are already global (row_base), its answer is the answer
        const size_t g = (size_t)sl->only_shard;
        if (rc == WAX_HIP_OK) rc = collect_impl(s->subs[g], sl->sub_tickets[g], out_ids, out_scores, capacity, out_count, nullptr, 0);
        else { uint32_t m = 0; wax_hip_hit tmp; (void)collect_impl(s->subs[g], sl->sub_tickets[g], nullptr, nullptr, 0, &m, &tmp, 0); }
    } else if (sl->host_path) {
        const size_t G = s->subs.size();
        const uint32_t limit = (uint32_t)clamp_topk(sl->top_k);
        static thread_local std::vector<wax_hip_hit> all, part;   // G x k keys: no allocation per query once warm
        all.clear();
        part.resize(limit);
        for (size_t g = 0; g < G; ++g) {
            if (sl->sub_tickets[g] == 0) continue;                // a shard without rows was not asked
            uint32_t m = 0;
            const int crc = collect_impl(s->subs[g], sl->sub_tickets[g], nullptr, nullptr, 0, &m, part.data(), limit);
            if (crc != WAX_HIP_OK && rc == WAX_HIP_OK) rc = crc;
            key_merge_add(all, part.data(), limit, KEY_PAD);
        }
        if (rc == WAX_HIP_OK) {
            // every part is sorted: the k best of G sorted runs (keys are unique: a total order, identical at any shard count)
            key_merge_cut(all, limit);
            rc = hits_to_results(e->metric, all.data(), (uint32_t)all.size(), out_ids, out_scores, capacity, out_count);
        }
    } else if (sl->kpad > 0 && rc == WAX_HIP_OK) {
        DeviceGuard dg(s->devices[0]);
        hipError_t err = hipEventSynchronize(sl->done);
        if (err != hipSuccess) rc = fail(WAX_HIP_ERR_INTERNAL, std::string("sharded search failed on device: ") + hipGetErrorString(err));
        else rc = hits_to_results(e->metric, sl->h_out, (uint32_t)sl->kpad, out_ids, out_scores, capacity, out_count);
    } else if (sl->kpad > 0) {
        DeviceGuard dg(s->devices[0]);
        (void)hipEventSynchronize(sl->done);
    }
    if (rc == WAX_HIP_OK && sl->has_cut && !sl->pred_deferred && out_ids && out_scores) apply_min_score(sl->cut, out_ids, out_scores, out_count);
    e->holders.note_collect(sl->owner);
    s->slots.release(sl);
    e->lock.unlock_shared();
    return rc;
}

// ---- batched search -----------------------------------------------------------------------------------------------------
//
// One batch on a sharded handle = one batch on every shard's own engine (its bf16 MFMA pipeline, exact re-score, shared
// exact pass for uncertified queries), all shards at once, then a per-query merge by key on the first device. Built on the
// single-device submit / collect pair, so ONE host thread drives all shards without blocking between them:
//   submit   per shard: query block -> the shard's device (peer copy on the shard's stream; skipped where the shard sits
//            on the caller's device), wax_hip_search_batch_submit_device (returns at once), and — enqueued on that batch's
//            own stream, i.e. right behind its last kernel — a peer copy of the shard's [nq][k] hits into the first
//            device's gather buffer + an event.
//   collect  per shard: collect its ticket (uncertified queries re-run exactly; if there were any, its part is copied
//            again), then the first device waits for the G events and merge_hits_kernel writes [nq][out_stride] hits.
// Workspaces are pooled per handle (query / hit buffers per shard, gather buffer, events): nothing is allocated and no
// thread is created per call. Nothing but nq x k hits per shard (and the queries, once) crosses xGMI.

void sh_free_bwork(ShardedState* s, ShardBatchWork* w) {
    if (!w) return;
    for (size_t g = 0; g < w->d_q.size(); ++g) {
        DeviceGuard dg(s->devices[g]);
        (void)hipFree(w->d_q[g]); (void)hipFree(w->d_part[g]);
        if (w->ev[g]) (void)hipEventDestroy(w->ev[g]);
    }
    DeviceGuard dg(s->devices[0]);
    (void)hipFree(w->d_all); (void)hipFree(w->d_q0); (void)hipFree(w->d_out0); (void)hipHostFree(w->h_out);
    if (w->ev_in) (void)hipEventDestroy(w->ev_in);
    if (w->done) (void)hipEventDestroy(w->done);
    delete w;
}

int sh_alloc_bwork(ShardedState* s, ShardBatchWork** out) {
    const size_t G = s->subs.size();
    ShardBatchWork* w = new ShardBatchWork();
    w->d_q.assign(G, nullptr); w->q_cap.assign(G, 0); w->d_part.assign(G, nullptr); w->part_cap.assign(G, 0);
    w->ev.assign(G, nullptr); w->sub_tickets.assign(G, 0); w->sub_valid.assign(G, 0);
    hipError_t err = hipSuccess;
    for (size_t g = 0; g < G && err == hipSuccess; ++g) {
        DeviceGuard dg(s->devices[g]);
        err = hipEventCreateWithFlags(&w->ev[g], hipEventDisableTiming);
    }
    if (err == hipSuccess) {
        DeviceGuard dg(s->devices[0]);
        err = hipEventCreateWithFlags(&w->ev_in, hipEventDisableTiming);
        if (err == hipSuccess) err = hipEventCreateWithFlags(&w->done, hipEventDisableTiming);
    }
    if (err != hipSuccess) {
        sh_free_bwork(s, w);
        return fail(WAX_HIP_ERR_ALLOC, std::string("Failed to allocate sharded batch workspace: ") + hipGetErrorString(err));
    }
    *out = w;
    return WAX_HIP_OK;
}

int sh_take_bwork(ShardedState* s, ShardBatchWork** out, bool try_only) {   // as take_bctx; returned by s->bworks.release(w)
    int rc = WAX_HIP_OK;
    const PoolGot got = s->bworks.acquire(try_only ? PoolMode::tries : PoolMode::wait, out, &rc, [s](int, ShardBatchWork** made) { return sh_alloc_bwork(s, made); });
    return got == PoolGot::busy ? fail(WAX_HIP_ERR_INVALID_ARGUMENT, kBatchWorkBusy) : rc;
}

// The stream a submitted single-device batch runs on (null: it was answered at submit time and is complete).
hipStream_t sh_batch_stream(wax_hip_engine* sub, uint64_t ticket) {
    hipStream_t st = nullptr;
    (void)sub->btickets.peek(ticket, [&st](const wax_hip_engine::BatchTicket& t) { if (t.c) st = t.c->stream; });
    return st;
}

int sh_copy_part(ShardedState* s, ShardBatchWork* w, size_t g, hipStream_t st) {
    const size_t n = (size_t)w->nq * w->k;
    DeviceGuard dg(s->devices[g]);
    hipError_t err = hipMemcpyPeerAsync(w->d_all + g * n, s->devices[0], w->d_part[g], s->devices[g], n * sizeof(wax_hip_hit), st);
    if (err == hipSuccess) err = hipEventRecord(w->ev[g], st);
    if (err != hipSuccess) return fail(WAX_HIP_ERR_INTERNAL, std::string("shard gather: ") + hipGetErrorString(err));
    return WAX_HIP_OK;
}

// Collect whatever sub-tickets a (failed or finished) batch still holds, so that every shard's read lock is released.
void sh_batch_drain(ShardedState* s, ShardBatchWork* w) {
    std::string keep = g_last_error;
    for (size_t g = 0; g < w->sub_valid.size(); ++g) {
        if (!w->sub_valid[g]) continue;
        DeviceGuard dg(s->devices[g]);
        (void)wax_hip_search_batch_collect_device(s->subs[g], w->sub_tickets[g], nullptr);
        w->sub_valid[g] = 0;
    }
    // the workspace goes back to the pool after this: nothing may still be landing in its gather / part buffers
    // (peer copies queued behind a shard's kernels, a merge already enqueued) when another batch picks it up
    for (size_t g = 0; g < s->subs.size(); ++g) {
        DeviceGuard dg(s->devices[g]);
        if (g < w->ev.size() && w->ev[g]) (void)hipEventSynchronize(w->ev[g]);
        (void)hipStreamSynchronize(s->streams[g]);
    }
    {
        DeviceGuard dg(s->devices[0]);
        (void)hipStreamSynchronize(s->merge_stream);
    }
    (void)hipGetLastError();
    g_last_error = keep;
}

// k = hits per query and shard (= rows of the gather buffer); the handle's shared lock is held by the caller.
int sh_batch_submit(wax_hip_engine* e, ShardBatchWork* w, const float* d_queries, uint32_t nq, uint32_t k, wax_hip_hit* d_out,
                    uint32_t out_stride, hipStream_t caller_stream) {
    ShardedState* s = e->sh;
    const size_t G = s->subs.size();
    const uint32_t dims = e->dims;
    const int dev0 = s->devices[0];
    w->d_queries = d_queries; w->d_out = d_out; w->nq = nq; w->k = k; w->out_stride = out_stride;
    std::fill(w->sub_valid.begin(), w->sub_valid.end(), 0);
    const uint64_t part = (uint64_t)nq * k;
    int rc = WAX_HIP_OK;
    {
        DeviceGuard dg(dev0);
        rc = grow_dev(&w->d_all, &w->all_cap, G * part, sizeof(wax_hip_hit), "Failed to allocate sharded gather buffer");
        if (rc != WAX_HIP_OK) return rc;
        HIP_TRY(hipEventRecord(w->ev_in, caller_stream), WAX_HIP_ERR_INTERNAL, "input event record");
    }
    auto one = [&](size_t g) -> int {
        const int dev = s->devices[g];
        DeviceGuard dg(dev);
        int r = grow_dev(&w->d_part[g], &w->part_cap[g], part, sizeof(wax_hip_hit), "Failed to allocate shard hit buffer");
        if (r != WAX_HIP_OK) return r;
        const float* qg = d_queries;
        hipStream_t producer = caller_stream;
        if (dev != dev0) {
            r = grow_dev(&w->d_q[g], &w->q_cap[g], (uint64_t)nq * dims, sizeof(float), "Failed to allocate shard query buffer");
            if (r != WAX_HIP_OK) return r;
            hipError_t err = hipStreamWaitEvent(s->streams[g], w->ev_in, 0);
            if (err == hipSuccess)
                err = hipMemcpyPeerAsync(w->d_q[g], dev, d_queries, dev0, (size_t)nq * dims * sizeof(float), s->streams[g]);
            if (err != hipSuccess) return fail(WAX_HIP_ERR_INTERNAL, std::string("query peer copy: ") + hipGetErrorString(err));
            qg = w->d_q[g];
            producer = s->streams[g];
        }
        r = wax_hip_search_batch_submit_device(s->subs[g], qg, nq, dims, (int32_t)k, w->d_part[g], k, producer, &w->sub_tickets[g]);
        if (r != WAX_HIP_OK) return r;
        w->sub_valid[g] = 1;
        hipStream_t bst = sh_batch_stream(s->subs[g], w->sub_tickets[g]);
        return sh_copy_part(s, w, g, bst ? bst : s->streams[g]);
    };
    // One host thread drives every shard when each shard's submit only ENQUEUES (the MFMA pipeline with a ready mirror). A
    // submit that would finish device work before returning — the loop path (dims % 64 != 0, k beyond the MFMA limits,
    // batch_mode = 0, small nq) or a mirror (re)build — goes to the persistent per-shard workers instead, so the shards
    // still run side by side rather than one after the other (a G-fold slowdown otherwise).
    bool blocks = false;
    for (size_t g = 0; g < G && G > 1 && !blocks; ++g) blocks = batch_submit_blocks(s->subs[g], dims, (int32_t)k, nq, k);
    rc = sh_fan_out(s, blocks ? FanOut::workers : FanOut::serial_stop, one);
    if (blocks) s->parallel_submits += 1;
    if (rc != WAX_HIP_OK) sh_batch_drain(s, w);
    return rc;
}

int sh_batch_collect(wax_hip_engine* e, ShardBatchWork* w, uint32_t* out_fallbacks) {
    ShardedState* s = e->sh;
    const size_t G = s->subs.size();
    uint32_t fallbacks = 0;
    std::vector<uint32_t> fbs(G, 0), rws(G, 0);
    // (every sub-ticket has to be collected, whatever another shard's collect returned)
    const bool parallel = G > 1 && s->collect_parallel.load() != 0;
    const int rc = sh_fan_out(s, parallel ? FanOut::workers : FanOut::serial_all, [&](size_t g) {
        if (!w->sub_valid[g]) return (int)WAX_HIP_OK;
        int crc = WAX_HIP_OK;
        {
            DeviceGuard dg(s->devices[g]);
            crc = batch_collect_device_impl(s->subs[g], w->sub_tickets[g], &fbs[g], &rws[g]);
        }
        w->sub_valid[g] = 0;
        // the part went to the first device right behind the shard's finish kernel; a full retry or the exact path has since
        // rewritten rows of it (synchronously, inside the collect above): send it again
        if (crc == WAX_HIP_OK && rws[g] > 0) crc = sh_copy_part(s, w, g, s->streams[g]);
        return crc;
    });
    if (parallel) s->parallel_collects += 1;
    int settled_on_host = 0;
    for (size_t g = 0; g < G; ++g) {
        fallbacks += fbs[g];
        settled_on_host += rws[g] > 0;
    }
    s->collect_parallel = settled_on_host >= 2 ? 1 : 0;
    if (out_fallbacks) *out_fallbacks = fallbacks;
    if (rc != WAX_HIP_OK) { sh_batch_drain(s, w); return rc; }   // also waits for the copies already in flight into w
    DeviceGuard dg(s->devices[0]);
    hipError_t err = hipSuccess;
    for (size_t g = 0; g < G && err == hipSuccess; ++g) err = hipStreamWaitEvent(s->merge_stream, w->ev[g], 0);
    const uint32_t nq = w->nq, k = w->k;
    if (err == hipSuccess) {
        if ((uint64_t)G * k <= 16384u && k <= (uint32_t)FUSED_MAX_K) {
            err = launch_merge_batch_hits(w->d_all, (uint32_t)G, nq, k, (int)k, w->d_out, s->merge_stream, w->out_stride);
            if (err == hipSuccess) err = hipEventRecord(w->done, s->merge_stream);
            if (err == hipSuccess) err = hipEventSynchronize(w->done);
        } else {
            // large k: merge on the host (the device merge serves k <= 192)
            std::vector<wax_hip_hit> all((size_t)G * nq * k), row, merged((size_t)nq * w->out_stride, wax_hip_hit{KEY_PAD, ID_PAD});
            err = hipStreamSynchronize(s->merge_stream);
            if (err == hipSuccess) err = hipMemcpy(all.data(), w->d_all, all.size() * sizeof(wax_hip_hit), hipMemcpyDeviceToHost);
            for (uint32_t q = 0; q < nq && err == hipSuccess; ++q) {
                row.clear();
                for (size_t g = 0; g < G; ++g) key_merge_add(row, all.data() + (g * nq + q) * (size_t)k, k, KEY_PAD);
                key_merge_cut(row, k);
                std::copy(row.begin(), row.end(), merged.begin() + (size_t)q * w->out_stride);
            }
            if (err == hipSuccess) err = hipMemcpy(w->d_out, merged.data(), merged.size() * sizeof(wax_hip_hit), hipMemcpyHostToDevice);
        }
    }
    if (err != hipSuccess) return fail(WAX_HIP_ERR_INTERNAL, std::string("sharded batch merge: ") + hipGetErrorString(err));
    return WAX_HIP_OK;
}

// Device-resident entry points on a sharded handle (queries and hits in the FIRST device's HBM). ticket == nullptr: blocking.
int sh_batch_device(wax_hip_engine* e, const float* d_queries, uint32_t nq, uint32_t dims, int32_t top_k, wax_hip_hit* d_out_hits,
                    uint32_t out_stride, void* stream, uint64_t* ticket) {
    ShardedState* s = e->sh;
    if (ticket) *ticket = 0;
    if (nq > 0 && (!d_queries || !d_out_hits || out_stride == 0)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null input");
    if (nq > 0 && dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));
    const bool holder = holding(e) > 0;
    e->lock.lock_shared(holder);
    bool keep_lock = false;
    struct Unlock { RWLock& l; bool& keep; ~Unlock() { if (!keep) l.unlock_shared(); } } unlock{e->lock, keep_lock};
    ShardBatchWork* w = nullptr;
    // a thread that already holds batch tickets must never WAIT for a workspace — it would wait for itself while holding the
    // handle's shared lock (and block every writer) — whether this call is a submit or a blocking search
    int rc = sh_take_bwork(s, &w, holder);
    if (rc != WAX_HIP_OK) return rc;
    bool keep_w = false;
    struct Release { ShardedState* s; ShardBatchWork* w; bool& keep; ~Release() { if (!keep) s->bworks.release(w); } } release{s, w, keep_w};
    std::fill(w->sub_valid.begin(), w->sub_valid.end(), 0);
    w->nq = 0;
    const uint64_t total = sh_count(s);
    uint64_t k64 = (uint64_t)clamp_topk(top_k);
    if (k64 > total) k64 = total;
    if (k64 > out_stride) k64 = out_stride;
    if (nq > 0 && k64 == 0) {   // empty engine: all padding
        DeviceGuard dg(s->devices[0]);
        std::vector<wax_hip_hit> pad((size_t)nq * out_stride, wax_hip_hit{KEY_PAD, ID_PAD});
        HIP_TRY(hipMemcpy(d_out_hits, pad.data(), pad.size() * sizeof(wax_hip_hit), hipMemcpyHostToDevice), WAX_HIP_ERR_INTERNAL, "pad upload");
    } else if (nq > 0) {
        rc = sh_batch_submit(e, w, d_queries, nq, (uint32_t)k64, d_out_hits, out_stride, static_cast<hipStream_t>(stream));
        if (rc != WAX_HIP_OK) return rc;
        if (!ticket) return sh_batch_collect(e, w, nullptr);
    }
    if (!ticket) return WAX_HIP_OK;
    e->holders.note_submit(&w->owner);
    *ticket = s->btickets.put(w);
    keep_w = true;
    keep_lock = true;
    return WAX_HIP_OK;
}

int sh_batch_collect_device(wax_hip_engine* e, uint64_t ticket, uint32_t* out_fallbacks) {
    ShardedState* s = e->sh;
    if (out_fallbacks) *out_fallbacks = 0;
    ShardBatchWork* w = nullptr;
    if (!s->btickets.take(ticket, &w)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "unknown batch ticket " + std::to_string(ticket));
    int rc = WAX_HIP_OK;
    if (w->nq > 0) {
        rc = sh_batch_collect(e, w, out_fallbacks);
        if (rc != WAX_HIP_OK) sh_batch_drain(s, w);
    }
    e->holders.note_collect(w->owner);
    s->bworks.release(w);
    e->lock.unlock_shared();
    return rc;
}

// nq queries -> nq rows of `stride` hits on the host: the queries go up to the first device once, the device-resident
// path above answers, the merged hits come down.
int sh_search_batch_hits(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k, wax_hip_hit* out_hits,
                         uint32_t stride, uint32_t* out_counts) {
    ShardedState* s = e->sh;
    for (uint32_t q = 0; q < nq; ++q) out_counts[q] = 0;
    for (size_t i = 0; i < (size_t)nq * stride; ++i) out_hits[i] = wax_hip_hit{KEY_PAD, ID_PAD};
    if (stride == 0 || nq == 0) return WAX_HIP_OK;
    if (dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));
    ReadGuard rd(e);
    const uint64_t total = sh_count(s);
    if (total == 0) return WAX_HIP_OK;
    uint32_t k = (uint32_t)clamp_topk(top_k);
    if (k > stride) k = stride;
    if ((uint64_t)k > total) k = (uint32_t)total;
    ShardBatchWork* w = nullptr;
    int rc = sh_take_bwork(s, &w, rd.holder);
    if (rc != WAX_HIP_OK) return rc;
    struct Release { ShardedState* s; ShardBatchWork* w; ~Release() { s->bworks.release(w); } } release{s, w};
    DeviceGuard dg(s->devices[0]);
    const uint64_t n_hits = (uint64_t)nq * k;
    rc = grow_dev(&w->d_q0, &w->q0_cap, (uint64_t)nq * dims, sizeof(float), "Failed to allocate batch queries");
    if (rc == WAX_HIP_OK) rc = grow_dev(&w->d_out0, &w->out0_cap, n_hits, sizeof(wax_hip_hit), "Failed to allocate batch hits");
    if (rc != WAX_HIP_OK) return rc;
    if (w->hout_cap < n_hits) {
        (void)hipHostFree(w->h_out);
        w->h_out = nullptr; w->hout_cap = 0;
        HIP_TRY(hipHostMalloc(&w->h_out, n_hits * sizeof(wax_hip_hit), hipHostMallocDefault), WAX_HIP_ERR_ALLOC, "Failed to allocate pinned batch hits");
        w->hout_cap = n_hits;
    }
    HIP_TRY(hipMemcpyAsync(w->d_q0, queries, (size_t)nq * dims * sizeof(float), hipMemcpyHostToDevice, s->merge_stream), WAX_HIP_ERR_INTERNAL, "query upload");
    rc = sh_batch_submit(e, w, w->d_q0, nq, k, w->d_out0, k, s->merge_stream);
    if (rc != WAX_HIP_OK) return rc;
    rc = sh_batch_collect(e, w, nullptr);
    if (rc != WAX_HIP_OK) { sh_batch_drain(s, w); return rc; }
    HIP_TRY(hipMemcpy(w->h_out, w->d_out0, n_hits * sizeof(wax_hip_hit), hipMemcpyDeviceToHost), WAX_HIP_ERR_INTERNAL, "hits download");
    for (uint32_t q = 0; q < nq; ++q) {
        uint32_t m = 0;
        for (uint32_t i = 0; i < k; ++i) {
            out_hits[(size_t)q * stride + i] = w->h_out[(size_t)q * k + i];
            m += w->h_out[(size_t)q * k + i].key != KEY_PAD;
        }
        out_counts[q] = m;
    }
    return WAX_HIP_OK;
}

// ---- filtered search: every shard pre-filters its own rows; the shards are in global row order, so a stable merge by
// (score desc, shard asc) is the (distance asc, global row asc) order of one engine (shard_merge.h: merge_by_score) -----

// One query on a handle: every shard answers on its own rows at the same time (persistent per-shard workers) through `per_shard`
// (shard engine, ids, scores, capacity, count) — the filtered or the predicate search — and the host merges them
// (merge_by_score) under the cut at clamp(top_k) and the caller's capacity.
template <typename PerShard>
static int sh_fanout_filtered(wax_hip_engine* e, uint32_t dims, int32_t top_k, uint64_t* out_ids, float* out_scores, uint32_t capacity,
                              uint32_t* out_count, PerShard per_shard, bool caller_locked = false) {
    ShardedState* s = e->sh;
    *out_count = 0;
    if (dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));
    // (caller_locked: the collect of a deferred predicate ticket, which holds the handle's shared lock itself)
    std::unique_ptr<ReadGuard> rd(caller_locked ? nullptr : new ReadGuard(e));
    const uint32_t limit = (uint32_t)clamp_topk(top_k);
    const size_t G = s->subs.size();
    std::vector<std::vector<uint64_t>> g_ids(G, std::vector<uint64_t>(limit));
    std::vector<std::vector<float>> g_scores(G, std::vector<float>(limit));
    std::vector<uint32_t> g_m(G, 0);
    const int rc = sh_fan_out(s, FanOut::workers, [&](size_t g) { return per_shard(s->subs[g], g_ids[g].data(), g_scores[g].data(), limit, &g_m[g]); });
    if (rc != WAX_HIP_OK) return rc;
    std::vector<ShardAnswer> parts(G);
    for (size_t g = 0; g < G; ++g) parts[g] = ShardAnswer{g_ids[g].data(), g_scores[g].data(), g_m[g]};
    std::vector<ShardHit> scratch;
    *out_count = merge_by_score(parts, limit, capacity, out_ids, out_scores, scratch);
    return WAX_HIP_OK;
}

int sh_search_filtered(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, int has_allow,
                       const uint64_t* allow, uint64_t n_allow, int has_min, float min_score, uint64_t* out_ids,
                       float* out_scores, uint32_t capacity, uint32_t* out_count) {
    // every shard pre-filters its own rows
    return sh_fanout_filtered(e, dims, top_k, out_ids, out_scores, capacity, out_count,
                              [&](wax_hip_engine* sub, uint64_t* ids, float* scores, uint32_t cap, uint32_t* n) {
                                  return wax_hip_search_filtered(sub, query, dims, top_k, has_allow, allow, n_allow, has_min, min_score, ids, scores, cap, n);
                              });
}

// The predicate search on a handle: every shard masks and searches its own rows (its attribute columns follow its rows).
int sh_search_predicate(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, int has_allow, const uint64_t* allow,
                        uint64_t n_allow, int has_min, float min_score, const wax_hip_row_predicate* pred, uint64_t* out_ids,
                        float* out_scores, uint32_t capacity, uint32_t* out_count, bool caller_locked) {
    return sh_fanout_filtered(e, dims, top_k, out_ids, out_scores, capacity, out_count,
                              [&](wax_hip_engine* sub, uint64_t* ids, float* scores, uint32_t cap, uint32_t* n) {
                                  return wax_hip_search_predicate(sub, query, dims, top_k, has_allow, allow, n_allow, has_min, min_score, pred, ids, scores, cap, n);
                              }, caller_locked);
}

// setAttributes / getAttributes on a handle: the ids are grouped by owning shard (call order kept inside a group, so the last entry
// of a repeated id still wins) and every shard that owns any is called once.
int sh_set_attributes(wax_hip_engine* e, const uint64_t* frame_ids, const int64_t* timestamps, const uint32_t* flags, uint64_t n,
                      uint64_t* out_applied) {
    ShardedState* s = e->sh;
    REFUSE_IF_HOLDING(e);
    WriteGuard w(e->lock);
    const std::vector<ShardRoute> per = sh_route(s, frame_ids, n);
    uint64_t total = 0;
    for (size_t g = 0; g < per.size(); ++g) {
        if (per[g].ids.empty()) continue;
        uint64_t got = 0;
        const std::vector<int64_t> ts = per[g].gather(timestamps);
        const std::vector<uint32_t> fl = per[g].gather(flags);
        const int rc = wax_hip_set_attributes(s->subs[g], per[g].ids.data(), timestamps ? ts.data() : nullptr, flags ? fl.data() : nullptr,
                                              per[g].ids.size(), &got);
        if (rc != WAX_HIP_OK) return rc;
        total += got;
    }
    if (out_applied) *out_applied = total;
    return WAX_HIP_OK;
}

int sh_get_attributes(wax_hip_engine* e, const uint64_t* frame_ids, uint64_t n, int64_t* out_ts, uint32_t* out_flags, uint8_t* out_found) {
    ShardedState* s = e->sh;
    ReadGuard rd(e);
    for (uint64_t i = 0; i < n; ++i) {
        if (out_ts) out_ts[i] = 0;
        if (out_flags) out_flags[i] = 0u;
        if (out_found) out_found[i] = 0;
    }
    const std::vector<ShardRoute> per = sh_route(s, frame_ids, n);
    for (size_t g = 0; g < per.size(); ++g) {
        const size_t m = per[g].ids.size();
        if (m == 0) continue;
        std::vector<int64_t> ts(m);
        std::vector<uint32_t> fl(m);
        std::vector<uint8_t> found(m);
        const int rc = wax_hip_get_attributes(s->subs[g], per[g].ids.data(), m, ts.data(), fl.data(), found.data());
        if (rc != WAX_HIP_OK) return rc;
        for (size_t j = 0; j < m; ++j) {
            const uint64_t i = per[g].at[j];
            if (out_ts) out_ts[i] = ts[j];
            if (out_flags) out_flags[i] = fl[j];
            if (out_found) out_found[i] = found[j];
        }
    }
    return WAX_HIP_OK;
}

// The timeline on a handle: every shard selects its own `limit` best rows (its columns follow its rows), side by side on the handle's
// workers; the host merges them by the same pair order — (timestamp, frame id), the timestamp reversed for newest-first — so the
// answer does not depend on which shard holds which frame.
int sh_timeline(wax_hip_engine* e, int32_t limit, int newest_first, const wax_hip_row_predicate* pred, uint64_t* out_ids, int64_t* out_ts,
                uint32_t capacity, uint32_t* out_count) {
    ShardedState* s = e->sh;
    *out_count = 0;
    ReadGuard rd(e);
    const size_t G = s->subs.size(), L = (size_t)limit;
    std::vector<uint64_t> g_ids(G * L);
    std::vector<int64_t> g_ts(G * L);
    std::vector<uint32_t> g_m(G, 0);
    const int rc = sh_fan_out(s, FanOut::workers, [&](size_t g) {
        return wax_hip_timeline(s->subs[g], limit, newest_first, pred, g_ids.data() + g * L, g_ts.data() + g * L, (uint32_t)limit, &g_m[g]);
    });
    if (rc != WAX_HIP_OK) return rc;
    *out_count = merge_timeline(g_ids.data(), g_ts.data(), g_m.data(), G, L, newest_first != 0, L, capacity, out_ids, out_ts);
    return WAX_HIP_OK;
}

// setParents / getParents on a handle: sh_set_attributes' routing — ids grouped by owning shard, call order kept inside a group.
int sh_set_parents(wax_hip_engine* e, const uint64_t* frame_ids, const uint64_t* parent_ids, uint64_t n, uint64_t* out_applied) {
    ShardedState* s = e->sh;
    REFUSE_IF_HOLDING(e);
    WriteGuard w(e->lock);
    const std::vector<ShardRoute> per = sh_route(s, frame_ids, n);
    uint64_t total = 0;
    for (size_t g = 0; g < per.size(); ++g) {
        if (per[g].ids.empty()) continue;
        uint64_t got = 0;
        const int rc = wax_hip_set_parents(s->subs[g], per[g].ids.data(), per[g].gather(parent_ids).data(), per[g].ids.size(), &got);
        if (rc != WAX_HIP_OK) return rc;
        total += got;
    }
    if (out_applied) *out_applied = total;
    return WAX_HIP_OK;
}

int sh_get_parents(wax_hip_engine* e, const uint64_t* frame_ids, uint64_t n, uint64_t* out_parents, uint8_t* out_found) {
    ShardedState* s = e->sh;
    ReadGuard rd(e);
    for (uint64_t i = 0; i < n; ++i) {
        if (out_parents) out_parents[i] = WAX_HIP_NO_PARENT;
        if (out_found) out_found[i] = 0;
    }
    const std::vector<ShardRoute> per = sh_route(s, frame_ids, n);
    for (size_t g = 0; g < per.size(); ++g) {
        const size_t m = per[g].ids.size();
        if (m == 0) continue;
        std::vector<uint64_t> parents(m);
        std::vector<uint8_t> found(m);
        const int rc = wax_hip_get_parents(s->subs[g], per[g].ids.data(), m, parents.data(), found.data());
        if (rc != WAX_HIP_OK) return rc;
        for (size_t j = 0; j < m; ++j) {
            if (out_parents) out_parents[per[g].at[j]] = parents[j];
            if (out_found) out_found[per[g].at[j]] = found[j];
        }
    }
    return WAX_HIP_OK;
}

// The grouped search on a handle, per_group == 1 (DESIGN 4.10): every shard answers `limit` groups on its own rows, side by side on the
// handle's workers; the host keeps the smaller distance per root (the lower shard on equal bits: shards are in global row order, so
// that is the lower row), sorts by (distance, root id) and takes `limit`. Exact: a root among the global first `limit` is, on the
// shard that holds its best row, beaten only by roots that beat it globally, so that shard returns it.
int sh_search_grouped(wax_hip_engine* e, const float* query, uint32_t dims, int32_t limit, int32_t per_group, int has_min_score, float min_score,
                      const wax_hip_row_predicate* pred, uint64_t* out_root_ids, float* out_root_scores, uint64_t* out_member_ids,
                      float* out_member_scores, uint32_t* out_member_counts, uint32_t* out_count) {
    ShardedState* s = e->sh;
    if (per_group > 1)
        return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "searchGrouped: per_group > 1 is not served on a sharded engine (a shard that did not rank a root cannot say what its members there are)");
    *out_count = 0;
    if (limit <= 0) return WAX_HIP_OK;
    ReadGuard rd(e);
    const bool members = out_member_ids != nullptr;
    const size_t G = s->subs.size();
    const uint32_t L = (uint32_t)limit, P = members ? 1u : 0u;
    std::vector<std::vector<int64_t>> raw(G);
    const int rc = sh_fan_out(s, FanOut::workers, [&](size_t g) { return grouped_raw(s->subs[g], query, dims, limit, (int32_t)P, pred, raw[g]); });
    if (rc != WAX_HIP_OK) return rc;
    GroupMerge merge;
    for (size_t g = 0; g < G; ++g) {
        const int64_t* r = raw[g].data();
        const uint32_t n = *reinterpret_cast<const uint32_t*>(r + 2u * (size_t)L);
        const int64_t* keys = r + 2u * (size_t)L + 1u;
        for (uint32_t i = 0; i < n && i < L; ++i)
            merge.offer((uint64_t)r[i], GroupBest{r[L + i], members ? keys[i] : KEY_PAD, members ? (uint64_t)keys[(size_t)L + i] : ID_PAD});
    }
    const std::vector<std::pair<int64_t, uint64_t>> order = merge.first(L);   // (signed distance bits, root id)
    uint32_t kept = 0;
    for (size_t i = 0; i < order.size(); ++i) {
        const float score = group_score(e->metric, unorder_bits((int32_t)order[i].first));
        if (has_min_score && score < min_score) continue;
        out_root_ids[kept] = order[i].second;
        out_root_scores[kept] = score;
        if (members) {
            const GroupBest& b = merge.best(order[i].second);
            out_member_ids[kept] = b.member;                 // (the group's own distance: it passed the cut with the group)
            out_member_scores[kept] = group_score(e->metric, key_distance(b.key));
        }
        if (out_member_counts) out_member_counts[kept] = members ? 1u : 0u;
        ++kept;
    }
    *out_count = kept;
    return WAX_HIP_OK;
}

int sh_group_stats(wax_hip_engine* e, wax_hip_group_stats_t* out) {
    *out = wax_hip_group_stats_t{};
    for (wax_hip_engine* sub : e->sh->subs) {
        wax_hip_group_stats_t one{};
        const int rc = wax_hip_group_stats(sub, &one);
        if (rc != WAX_HIP_OK) return rc;
        out->searches += one.searches; out->fused_scans += one.fused_scans; out->column_scans += one.column_scans;
        out->member_rounds += one.member_rounds; out->group_slots += one.group_slots; out->parent_rows_uploaded += one.parent_rows_uploaded;
    }
    return WAX_HIP_OK;
}

// setTerms / getTerms on a handle: sh_set_parents' routing — the entries of the validated plan go to the shard that owns their frame.
// Every shard's total is checked before any shard is changed: a refusal leaves the whole handle as it was.
int sh_set_terms(wax_hip_engine* e, const uint64_t* frame_ids, uint64_t n, const TermPlan& plan, uint64_t* out_applied) {
    ShardedState* s = e->sh;
    REFUSE_IF_HOLDING(e);
    WriteGuard w(e->lock);
    const size_t G = s->subs.size();
    const std::vector<ShardRoute> per = sh_route(s, frame_ids, n);
    std::vector<TermRows> rows(G);
    uint64_t applied = 0;
    for (size_t g = 0; g < G; ++g) {
        applied += per[g].at.size();
        for (size_t j = 0; j < per[g].at.size(); ++j) rows[g].emplace_back(per[g].rows[j], per[g].at[j]);
    }
    std::vector<std::unique_ptr<WriteGuard>> sub_locks;        // (in shard order; searches of the shards' workers hold their shared locks)
    for (size_t g = 0; g < G; ++g) {
        if (rows[g].empty()) continue;
        finish_term_rows(&rows[g]);
        sub_locks.emplace_back(new WriteGuard(s->subs[g]->lock));
        if (s->subs[g]->cols.terms().total_after(plan, rows[g]) >= 0x100000000ull)
            return fail(WAX_HIP_ERR_CAPACITY, "setTerms: a shard would hold 2^32 terms or more");
    }
    for (size_t g = 0; g < G; ++g)
        if (!rows[g].empty()) s->subs[g]->cols.commit_terms(plan, rows[g]);
    if (out_applied) *out_applied = applied;
    return WAX_HIP_OK;
}

int sh_get_terms(wax_hip_engine* e, uint64_t frame_id, uint32_t* out_terms, uint32_t out_capacity, uint32_t* out_count, uint8_t* out_found) {
    ShardedState* s = e->sh;
    ReadGuard rd(e);
    int64_t local = -1;
    const int g = sh_find(s, frame_id, &local);
    if (g < 0) return WAX_HIP_OK;
    return wax_hip_get_terms(s->subs[(size_t)g], frame_id, out_terms, out_capacity, out_count, out_found);
}

// The term search on a handle: every shard masks and searches its own rows (its term column follows its rows).
int sh_search_terms(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, int has_allow, const uint64_t* allow, uint64_t n_allow,
                    int has_min, float min_score, const wax_hip_row_predicate* pred, const uint32_t* required, uint32_t n_required,
                    uint64_t* out_ids, float* out_scores, uint32_t capacity, uint32_t* out_count) {
    return sh_fanout_filtered(e, dims, top_k, out_ids, out_scores, capacity, out_count,
                              [&](wax_hip_engine* sub, uint64_t* ids, float* scores, uint32_t cap, uint32_t* n) {
                                  return wax_hip_search_terms(sub, query, dims, top_k, has_allow, allow, n_allow, has_min, min_score, pred, required,
                                                              n_required, ids, scores, cap, n);
                              });
}

int sh_term_stats(wax_hip_engine* e, wax_hip_term_stats_t* out) {
    *out = wax_hip_term_stats_t{};
    for (wax_hip_engine* sub : e->sh->subs) {
        wax_hip_term_stats_t one{};
        const int rc = wax_hip_term_stats(sub, &one);
        if (rc != WAX_HIP_OK) return rc;
        out->searches += one.searches; out->device_masks += one.device_masks; out->host_staged += one.host_staged;
        out->host_decided += one.host_decided; out->term_rows_uploaded += one.term_rows_uploaded; out->term_values_uploaded += one.term_values_uploaded;
    }
    return WAX_HIP_OK;
}

int sh_term_batch_stats(wax_hip_engine* e, wax_hip_term_batch_stats_t* out) {
    *out = wax_hip_term_batch_stats_t{};
    for (wax_hip_engine* sub : e->sh->subs) {
        wax_hip_term_batch_stats_t one{};
        const int rc = wax_hip_term_batch_stats(sub, &one);
        if (rc != WAX_HIP_OK) return rc;
        out->calls += one.calls; out->queries += one.queries; out->sets += one.sets; out->mask_launches += one.mask_launches;
        out->looped += one.looped; out->host_decided += one.host_decided;
    }
    return WAX_HIP_OK;
}

// Batched form: every shard answers the whole batch on its own rows (its own batched filtered call, on the handle's workers, in
// parallel); then each query is merged exactly as sh_search_filtered merges one: stable by score, shard order on ties, then the cut.
// preds (null: none) go to every shard as they are: a row's attributes live with the shard that owns the row.
int sh_search_batch_predicate(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k, const uint64_t* allow,
                              uint64_t n_allow_ids, const uint64_t* allow_begin, const uint64_t* allow_len, const float* min_scores,
                              const wax_hip_row_predicate* preds, uint64_t* out_ids, float* out_scores, uint32_t out_stride, uint32_t* out_counts,
                              const uint32_t* required_terms, uint64_t n_required_terms, const uint64_t* term_begin, const uint32_t* term_len) {
    ShardedState* s = e->sh;
    if (dims != e->dims) return fail(WAX_HIP_ERR_DIM_MISMATCH, dim_mismatch_msg(e->dims, dims));
    if (out_stride == 0) return WAX_HIP_OK;
    ReadGuard rd(e);
    const uint32_t limit = (uint32_t)clamp_topk(top_k);
    const size_t G = s->subs.size();
    std::vector<std::vector<uint64_t>> g_ids(G, std::vector<uint64_t>((size_t)nq * limit));
    std::vector<std::vector<float>> g_scores(G, std::vector<float>((size_t)nq * limit));
    std::vector<std::vector<uint32_t>> g_m(G, std::vector<uint32_t>(nq, 0));
    const int rc = sh_fan_out(s, FanOut::workers, [&](size_t g) {
        // (term_begin / term_len null: wax_hip_search_batch_predicate itself; a row's terms live with the shard that owns the row)
        return wax_hip_search_batch_terms(s->subs[g], queries, nq, dims, top_k, allow, n_allow_ids, allow_begin, allow_len, nullptr, preds,
                                          required_terms, n_required_terms, term_begin, term_len, g_ids[g].data(), g_scores[g].data(), limit,
                                          g_m[g].data());
    });
    if (rc != WAX_HIP_OK) return rc;
    std::vector<ShardAnswer> parts(G);
    std::vector<ShardHit> scratch;
    for (uint32_t q = 0; q < nq; ++q) {
        for (size_t g = 0; g < G; ++g) parts[g] = ShardAnswer{g_ids[g].data() + (size_t)q * limit, g_scores[g].data() + (size_t)q * limit, g_m[g][q]};
        uint64_t* ids = out_ids + (size_t)q * out_stride;
        float* scores = out_scores + (size_t)q * out_stride;
        uint32_t m = merge_by_score(parts, limit, out_stride, ids, scores, scratch);
        if (min_scores) apply_min_score(min_scores[q], ids, scores, &m);
        out_counts[q] = m;
    }
    return WAX_HIP_OK;
}

// ---- persistence ------------------------------------------------------------------------------------------------------------

int sh_serialize(wax_hip_engine* e, uint8_t** out_bytes, size_t* out_len) {
    ShardedState* s = e->sh;
    ReadGuard rd(e);                                                        // withReadLock (MetalVectorEngine.swift:683)
    for (auto* sub : s->subs) { const int frc = flush_pending(sub); if (frc != WAX_HIP_OK) return frc; }
    const uint64_t n = sh_count(s);
    const uint64_t vec_bytes = n * (uint64_t)e->dims * 4ull, id_bytes = n * 8ull;
    const size_t total = 36 + (size_t)vec_bytes + 8 + (size_t)id_bytes;
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(total));
    if (!buf) return fail(WAX_HIP_ERR_ALLOC, "Failed to allocate serialize buffer");
    uint8_t* p = buf;
    const uint8_t magic[4] = {0x4D, 0x56, 0x32, 0x56};
    std::memcpy(p, magic, 4); p += 4;
    const uint16_t ver = 1; std::memcpy(p, &ver, 2); p += 2;
    *p++ = 2; *p++ = e->metric;
    std::memcpy(p, &e->dims, 4); p += 4;
    std::memcpy(p, &n, 8); p += 8;
    std::memcpy(p, &vec_bytes, 8); p += 8;
    std::memset(p, 0, 8); p += 8;
    int rc = WAX_HIP_OK;
    for (size_t g = 0; g < s->subs.size() && rc == WAX_HIP_OK; ++g) {     // shards in order = global row order
        wax_hip_engine* sub = s->subs[g];
        const size_t bytes = (size_t)sub->count * e->dims * 4;
        if (bytes) {
            DeviceGuard dg(s->devices[g]);
            hipError_t err = hipMemcpy(p, sub->d_store, bytes, hipMemcpyDeviceToHost);
            if (err != hipSuccess) rc = fail(WAX_HIP_ERR_INTERNAL, std::string("vector download: ") + hipGetErrorString(err));
        }
        p += bytes;
    }
    std::memcpy(p, &id_bytes, 8); p += 8;
    for (auto* sub : s->subs) { std::memcpy(p, sub->ids.data(), (size_t)sub->count * 8); p += (size_t)sub->count * 8; }
    if (rc != WAX_HIP_OK) { std::free(buf); return rc; }
    *out_bytes = buf;
    *out_len = total;
    return WAX_HIP_OK;
}

int sh_deserialize(wax_hip_engine* e, const uint8_t* data, size_t len) {
    ShardedState* s = e->sh;
    uint64_t n = 0, vec_len = 0, id_len = 0;   // header validation: the single-device engine's (same order and reasons, :716-808)
    { const int vrc = validate_mv2v_segment(e->metric, e->dims, data, len, &n, &vec_len, &id_len); if (vrc != WAX_HIP_OK) return vrc; }
    const uint32_t dims = e->dims;
    REFUSE_IF_HOLDING(e);
    WriteGuard w(e->lock);
    const size_t G = s->subs.size();
    s->layout.segment(sh_shape(s, dims), n);   // (a segment below "shard_min_mb" loads into the first shard alone)
    const uint8_t* vec = data + 36;
    const uint8_t* idp = data + 36 + vec_len + 8;
    int rc = WAX_HIP_OK;
    for (size_t g = 0; g < G && rc == WAX_HIP_OK; ++g) {
        uint64_t lo = 0, hi = 0;
        s->layout.slice(g, n, &lo, &hi);
        const uint64_t m = hi - lo;
        // the shard's slice as a segment of its own: the single-device deserialize keeps its exact semantics
        // (duplicate ids stay separate rows, first row wins the id map, :809-811)
        std::vector<uint8_t> seg(36 + (size_t)m * dims * 4 + 8 + (size_t)m * 8);
        uint8_t* p = seg.data();
        std::memcpy(p, data, 12); p += 12;
        std::memcpy(p, &m, 8); p += 8;
        const uint64_t vb = m * (uint64_t)dims * 4ull, ib = m * 8ull;
        std::memcpy(p, &vb, 8); p += 8;
        std::memset(p, 0, 8); p += 8;
        std::memcpy(p, vec + lo * (uint64_t)dims * 4ull, (size_t)vb); p += vb;
        std::memcpy(p, &ib, 8); p += 8;
        std::memcpy(p, idp + lo * 8ull, (size_t)ib);
        rc = wax_hip_deserialize(s->subs[g], seg.data(), seg.size());
    }
    sh_update_bases(s);
    return rc;
}

uint64_t sh_total_count(const wax_hip_engine* e) { return sh_count(e->sh); }

int sh_stats(wax_hip_engine* e, wax_hip_stats_t* out) {
    std::memset(out, 0, sizeof(*out));
    for (auto* sub : e->sh->subs) {
        wax_hip_stats_t t{};
        int rc = wax_hip_stats(sub, &t);
        if (rc != WAX_HIP_OK) return rc;
        out->searches += t.searches; out->rows_scanned += t.rows_scanned; out->bytes_scanned += t.bytes_scanned;
        out->transient_allocations += t.transient_allocations; out->reuse_count += t.reuse_count; out->reserved_rows += t.reserved_rows;
        out->scan_kernel_ms_total += t.scan_kernel_ms_total; out->scan_kernels_timed += t.scan_kernels_timed;
        out->last_scan_kernel_ms = std::max(out->last_scan_kernel_ms, t.last_scan_kernel_ms);
        out->batch_gemm_ms_total += t.batch_gemm_ms_total; out->batch_gemms_timed += t.batch_gemms_timed;
        out->batch_gemm_rows += t.batch_gemm_rows; out->batch_gemm_queries += t.batch_gemm_queries;
    }
    return WAX_HIP_OK;
}

int sh_set_tuning(wax_hip_engine* e, const std::string& k, int64_t value) {
    ShardedState* s = e->sh;
    if (k == "exchange") {   // 0 = peer copies of the k hits + merge on the first device (default), 1 = RCCL all-gather per query
        if (value != 0 && value != 1) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "exchange must be 0 (peer copy) or 1 (rccl)");
        if (value == 1) {
            REFUSE_IF_HOLDING(e);     // (a thread with uncollected tickets holds the shared lock: it would wait for itself)
            WriteGuard w(e->lock);
            int rc = sh_load_rccl(s);
            if (rc != WAX_HIP_OK) return rc;
        }
        s->exchange = value;
        return WAX_HIP_OK;
    }
    if (k == "gather") {     // 0 = device gather (peer copies / rccl) + merge on the first device; 2 = host-staged gather + host merge
        if (value != 0 && value != 2) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "gather must be 0 (device) or 2 (host-staged)");
        if (value == 0 && s->peer_enabled < s->peer_pairs)
            return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "device gather needs peer access between device " + std::to_string(s->devices[0]) +
                                                          " and every shard device (" + std::to_string(s->peer_enabled) + " of " +
                                                          std::to_string(s->peer_pairs) + " pairs have it)");
        REFUSE_IF_HOLDING(e);
        WriteGuard w(e->lock);
        s->host_gather = value == 2;
        return WAX_HIP_OK;
    }
    if (k == "ticket_path") {   // single-query searches: 1 = per-shard tickets submitted side by side + host merge (default), 0 = device gather
        if (value != 0 && value != 1) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "ticket_path must be 0 or 1");
        s->ticket_path = value;
        return WAX_HIP_OK;
    }
    if (k == "shard_min_mb") {  // a shard's block holds at least this many MB of rows (0 = spread from the first row); takes effect when the layout is next chosen
        if (value < 0 || value > (1 << 20)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "shard_min_mb must be 0..1048576");
        REFUSE_IF_HOLDING(e);
        WriteGuard w(e->lock);
        s->shard_min_mb = value;
        if (sh_count(s) == 0) s->layout.block_rows = 0;                  // an empty handle chooses again at its first rows / reserve
        return WAX_HIP_OK;
    }
    for (auto* sub : s->subs) {   // everything else is a per-shard setting, checked by its row (tuning.inc)
        int rc = wax_hip_set_tuning(sub, k.c_str(), value);
        if (rc != WAX_HIP_OK) return rc;
    }
    if (k == "batch_workspaces") s->bworks.set_cap((int)value);   // concurrent batched searches per shard (above) and per handle
    return WAX_HIP_OK;
}

int64_t sh_get_tuning(wax_hip_engine* e, const std::string& k) {
    ShardedState* s = e->sh;
    if (k == "exchange") return s->exchange.load();
    if (k == "shards") return (int64_t)s->subs.size();
    if (k == "gather") return s->host_gather ? 2 : 0;
    if (k == "peer_pairs") return s->peer_pairs;
    if (k == "peer_enabled") return s->peer_enabled;
    if (k == "rccl_ranks") {   // ranks of the single-process communicator as RCCL itself counts them (0 = no communicator)
        if (s->comms.empty() || !s->comms[0]) return 0;
        int n = 0;
        if (s->rccl.CommCount && s->rccl.CommCount(s->comms[0], &n) == 0) return n;
        return (int64_t)s->comms.size();
    }
    if (k == "block_rows") return (int64_t)s->layout.block_rows;
    if (k == "ticket_path") return s->ticket_path.load();
    if (k == "shard_min_mb") return s->shard_min_mb.load();
    if (k == "ticket_searches") return (int64_t)s->ticket_searches.load();
    if (k == "single_shard_searches") return (int64_t)s->single_shard_searches.load();
    if (k == "inline_fanouts") return (int64_t)s->inline_fanouts.load();   // single-query fan-outs submitted from the caller's thread because the workers were busy
    if (k == "rccl_collectives") return (int64_t)s->rccl_collectives.load();
    if (k == "rebalances") return (int64_t)s->rebalances.load();
    if (k == "parallel_collects") return (int64_t)s->parallel_collects.load();
    if (k == "parallel_submits") return (int64_t)s->parallel_submits.load();
    const TuningRow* row = tuning_row(k);   // tuning.inc: a shard's keys and what the handle answers for each
    if (row && row->sharded == SUM_SHARDS) {
        int64_t t = 0;
        for (auto* sub : s->subs) t += wax_hip_get_tuning(sub, k.c_str());
        return t;
    }
    return wax_hip_get_tuning(s->subs[0], k.c_str());
}

void sh_destroy(wax_hip_engine* e) {
    ShardedState* s = e->sh;
    for (size_t g = 0; g < s->subs.size(); ++g) {
        DeviceGuard dg(s->devices[g]);
        (void)hipDeviceSynchronize();
    }
    s->workers.stop();
    s->slots.drain([s](ShardSlot* sl) { sh_free_slot(s, sl); });
    s->bworks.drain([s](ShardBatchWork* w) { sh_free_bwork(s, w); });
    if (s->rccl.lib && s->rccl.CommDestroy)
        for (void* c : s->comms)
            if (c) (void)s->rccl.CommDestroy(c);
    for (size_t g = 0; g < s->streams.size(); ++g) {
        DeviceGuard dg(s->devices[g]);
        if (s->streams[g]) (void)hipStreamDestroy(s->streams[g]);
    }
    if (s->merge_stream) { DeviceGuard dg(s->devices[0]); (void)hipStreamDestroy(s->merge_stream); }
    for (auto* sub : s->subs) wax_hip_engine_destroy(sub);
    delete s;
    e->sh = nullptr;
}

}  // namespace

// ===========================================================================
extern "C" {

int wax_hip_engine_create_sharded(uint8_t metric, uint32_t dims, const int* device_ids, int n_devices, wax_hip_engine** out) {
    if (!out) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    if (!device_ids || n_devices < 1 || n_devices > 64) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "device list must name 1..64 devices");
    const int visible = wax_hip_device_count();
    for (int i = 0; i < n_devices; ++i)
        if (device_ids[i] < 0 || device_ids[i] >= visible)
            return fail(WAX_HIP_ERR_NO_DEVICE, "HIP device " + std::to_string(device_ids[i]) + " not available (" + std::to_string(visible) + " visible)");
    wax_hip_engine* e = new wax_hip_engine();
    e->metric = metric;
    e->dims = dims;
    e->device = device_ids[0];
    ShardedState* s = new ShardedState();
    e->sh = s;
    int rc = WAX_HIP_OK;
    for (int i = 0; i < n_devices && rc == WAX_HIP_OK; ++i) {
        wax_hip_engine* sub = nullptr;
        rc = wax_hip_engine_create(metric, dims, device_ids[i], &sub);     // validates metric / dims / gfx950 like a single engine
        if (rc != WAX_HIP_OK) break;
        s->subs.push_back(sub);
        s->devices.push_back(device_ids[i]);
        DeviceGuard dg(device_ids[i]);
        hipStream_t st = nullptr;
        hipError_t err = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        if (err != hipSuccess) { rc = fail(WAX_HIP_ERR_ALLOC, std::string("Failed to create stream: ") + hipGetErrorString(err)); break; }
        s->streams.push_back(st);
    }
    if (rc == WAX_HIP_OK) {
        DeviceGuard dg(s->devices[0]);
        hipError_t err = hipStreamCreateWithFlags(&s->merge_stream, hipStreamNonBlocking);
        if (err != hipSuccess) rc = fail(WAX_HIP_ERR_ALLOC, std::string("Failed to create stream: ") + hipGetErrorString(err));
    }
    if (rc == WAX_HIP_OK) {
        // Peer access for the k-hit gather and the query broadcast: first device <-> every other shard device, checked and
        // enabled per pair and per direction. A pair without it is reported (stderr, "peer_enabled" / "peer_pairs"); the
        // handle then gathers through the host ("gather" = 2: per-shard D2H of k hits + host merge, bit-identical results)
        // instead of trusting implicit staging — or refuses to exist when WAX_HIP_REQUIRE_PEER=1.
        std::string missing;
        for (size_t g = 1; g < s->devices.size(); ++g) {
            const int a = s->devices[0], b = s->devices[g];
            if (a == b) continue;
            bool dup = false;
            for (size_t h = 1; h < g; ++h) dup = dup || s->devices[h] == b;
            if (dup) continue;
            s->peer_pairs++;
            bool ok = true;
            for (int dir = 0; dir < 2 && ok; ++dir) {
                const int from = dir ? b : a, to = dir ? a : b;
                int can = 0;
                hipError_t perr = hipDeviceCanAccessPeer(&can, from, to);
                if (perr != hipSuccess || !can) { (void)hipGetLastError(); ok = false; break; }
                DeviceGuard dg(from);
                perr = hipDeviceEnablePeerAccess(to, 0);
                if (perr == hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); perr = hipSuccess; }
                if (perr != hipSuccess) { (void)hipGetLastError(); ok = false; }
            }
            if (ok) s->peer_enabled++;
            else missing += (missing.empty() ? "" : ", ") + std::to_string(a) + "<->" + std::to_string(b);
        }
        if (s->peer_enabled < s->peer_pairs) {
            const char* req = std::getenv("WAX_HIP_REQUIRE_PEER");
            if (req && req[0] == '1')
                rc = fail(WAX_HIP_ERR_NO_DEVICE, "no peer access between HIP devices " + missing + " (WAX_HIP_REQUIRE_PEER=1)");
            else {
                s->host_gather = true;
                // (single-query searches then never touch a peer API: per-shard tickets, hits to pinned memory, host merge. BATCHED
                // searches still move the query block and the [nq][k] hit parts with hipMemcpyPeerAsync, which the runtime stages
                // through the host when the devices cannot reach each other directly — correct, slower; WAX_HIP_REQUIRE_PEER=1 is
                // the strict setting)
                std::fprintf(stderr, "[wax_hip] sharded engine: no peer access between devices %s; single-query hits are gathered "
                                     "through the host, batched searches use runtime-staged peer copies (set WAX_HIP_REQUIRE_PEER=1 "
                                     "to fail instead)\n", missing.c_str());
            }
        }
    }
    if (rc != WAX_HIP_OK) {
        std::string keep = g_last_error;
        wax_hip_engine_destroy(e);
        g_last_error = keep;
        return rc;
    }
    if (const char* v = std::getenv("WAX_HIP_SHARD_MIN_MB")) {   // default of "shard_min_mb" (tests that want small stores spread over every shard set 0)
        const long mb = std::strtol(v, nullptr, 10);
        if (mb >= 0 && mb <= (1 << 20)) s->shard_min_mb = mb;
    }
    s->workers.start(s->devices.size(), [s](size_t g) { (void)hipSetDevice(s->devices[g]); });
    *out = e;
    return WAX_HIP_OK;
}

int wax_hip_shard_count(const wax_hip_engine* e) { return e ? (e->sh ? (int)e->sh->subs.size() : 1) : 0; }

int wax_hip_shard_info(const wax_hip_engine* e, int shard, int* out_device, uint64_t* out_row_base, uint64_t* out_rows) {
    if (!e) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "engine is null");
    const int n = wax_hip_shard_count(e);
    if (shard < 0 || shard >= n) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "shard index out of range");
    const wax_hip_engine* sub = e->sh ? e->sh->subs[(size_t)shard] : e;
    if (out_device) *out_device = sub->device;
    if (out_row_base) *out_row_base = sub->row_base;
    if (out_rows) *out_rows = sub->count;
    return WAX_HIP_OK;
}

}  // extern "C"
