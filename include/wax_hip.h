/*
 * wax_hip.h — C ABI of libwaxhip: the MI355X (gfx950 / CDNA4) brute-force vector
 * scan + top-k backend for Wax's `VectorSearchEngine`.
 *
 * This is the drop-in boundary. Every entry point replaces one
 * member of the reference's Swift surface; the reference file:line it stands in
 * for is cited on each declaration (paths relative to the reference checkout).
 * A Swift `actor HIPVectorEngine: VectorSearchEngine` binds these through a
 * module map; Python binds them with ctypes
 * (wax_amd/_abi.py); C++ callers can use include/wax_hip.hpp.
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in any signature
 *     (`void* stream` is a hipStream_t passed opaquely, NULL = engine's own)
 *   - return 0 (WAX_HIP_OK) or a negative wax_hip_status; the message is in
 *     wax_hip_last_error() (thread-local)
 *   - the caller owns every in/out array and states its size: every result array comes with an
 *     explicit capacity (entries) and the library never writes past it, whatever the engine's row
 *     count has become by the time the call runs (a concurrent add may grow it between the caller's
 *     sizing and the search). wax_hip_result_capacity(top_k) = clamp(top_k, 1, 10000) entries always
 *     suffice. Buffers returned by wax_hip_serialize() are released with wax_hip_free()
 *   - search* calls are re-entrant (shared lock + per-call scratch slot),
 *     mutations take the exclusive lock — the same reader/writer contract as
 *     the reference's AsyncReadWriteLock (MetalVectorEngine.swift:56-81)
 *   - there is NO CPU fallback in this library: without a gfx950 device every
 *     engine call fails with WAX_HIP_ERR_NO_DEVICE.
 */
#ifndef WAX_HIP_H
#define WAX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WAX_HIP_ABI_VERSION 2

/* MetalVectorEngine.maxResults (MetalVectorEngine.swift:18) */
#define WAX_HIP_MAX_RESULTS 10000
/* Constants.maxEmbeddingDimensions (WaxCore/Constants.swift:51) */
#define WAX_HIP_MAX_DIMENSIONS 1000000
/* MetalVectorEngine.initialReserve (MetalVectorEngine.swift:19) */
#define WAX_HIP_INITIAL_RESERVE 64

typedef struct wax_hip_engine wax_hip_engine;

/* Maps 1:1 onto the WaxError cases the Metal engine throws
 * (MetalVectorEngine.swift:154-169, 830-840, 858-860; WaxError.swift:4-18). */
typedef enum wax_hip_status {
    WAX_HIP_OK = 0,
    WAX_HIP_ERR_DIM_MISMATCH = -1,      /* WaxError.encodingError("vector dimension mismatch: expected X, got Y") */
    WAX_HIP_ERR_CAPACITY = -2,          /* WaxError.capacityExceeded(limit:requested:) */
    WAX_HIP_ERR_NO_DEVICE = -3,         /* WaxError.invalidToc("... device not available") */
    WAX_HIP_ERR_ALLOC = -4,             /* WaxError.invalidToc("Failed to allocate ...") */
    WAX_HIP_ERR_BAD_SEGMENT = -5,       /* WaxError.invalidToc(<segment decode reason>) */
    WAX_HIP_ERR_METRIC_UNSUPPORTED = -6,
    WAX_HIP_ERR_INVALID_ARGUMENT = -7,  /* WaxError.encodingError / invalidToc("dimensions must be > 0") */
    WAX_HIP_ERR_INTERNAL = -8
} wax_hip_status;

/* VecSimilarity raw values (WaxCore/FileFormat/MV2SEnums.swift:34-38) ==
 * VectorMetric cases (VectorMetric.swift:5-8). */
typedef enum wax_hip_metric {
    WAX_HIP_METRIC_COSINE = 0,
    WAX_HIP_METRIC_DOT = 1,
    WAX_HIP_METRIC_L2 = 2
} wax_hip_metric;

/* One ranked candidate as it lives in HBM and travels over RCCL between shards.
 * key = (int64)ordered(distance_f32) << 32 | global_row_u32, where ordered()
 * is the sign-magnitude -> two's-complement monotone map, so that a SIGNED
 * 64-bit ascending sort is exactly "(distance asc, row asc)" — the tie rule
 * SURVEY.md §8c adopts from MetalVectorEngine.topK's earlier-index-wins
 * boundary (MetalVectorEngine.swift:671). Replaces the reference's
 * TopKEntry{float distance; uint index} (TopKReduction.metal:15-18,
 * MetalVectorEngine.swift:26-29) plus the frameIds[index] lookup (:601). */
typedef struct wax_hip_hit {
    int64_t key;
    uint64_t frame_id;
} wax_hip_hit;

/* Counters; superset of MetalVectorEngine.BufferPoolStats
 * (MetalVectorEngine.swift:43-46, 119-121). */
typedef struct wax_hip_stats_t {
    uint64_t searches;             /* single-query scans issued */
    uint64_t rows_scanned;         /* sum of rows visited by those scans */
    uint64_t bytes_scanned;        /* algorithmic bytes: rows * dims * 4 */
    uint64_t transient_allocations;/* scratch slots created (BufferPoolStats.transientAllocations) */
    uint64_t reuse_count;          /* scratch slot reuses (BufferPoolStats.reuseCount) */
    uint64_t reserved_rows;        /* current capacity in rows (reservedCapacity) */
    double   last_scan_kernel_ms;  /* HIP-event time of the most recent timed scan kernel (0 if timing off) */
    double   scan_kernel_ms_total; /* sum of HIP-event scan-kernel times since "reset_stats" ("time_kernels"=1) */
    uint64_t scan_kernels_timed;   /* number of scan-kernel launches in that sum */
    double   batch_gemm_ms_total;  /* sum of HIP-event times of the batched path's filtering GEMM launches ("time_kernels"=1) */
    uint64_t batch_gemms_timed;    /* number of GEMM launches in that sum */
    uint64_t batch_gemm_rows;      /* corpus rows those launches covered, summed (algorithmic bytes = rows * dims * 2, bf16 mirror) */
    uint64_t batch_gemm_queries;   /* queries those launches served, summed (flops = 2 * queries * rows-per-launch * dims) */
} wax_hip_stats_t;

/* ---- availability ------------------------------------------------------- */

/* MetalVectorEngine.isAvailable (MetalVectorEngine.swift:144-146): 1 iff a gfx950 device is visible. */
int wax_hip_available(void);
int wax_hip_device_count(void);
uint32_t wax_hip_abi_version(void);
/* thread-local, never NULL */
const char* wax_hip_last_error(void);

/* ---- lifecycle ---------------------------------------------------------- */

/* MetalVectorEngine.init(metric:dimensions:) (MetalVectorEngine.swift:153-274).
 * metric: wax_hip_metric (the Metal engine accepts only cosine, :163-165; this
 * backend also implements dot and l2 with USearch's distance conventions,
 * VectorMetric.swift:21-43). device_id: HIP ordinal, -1 = current device. */
int wax_hip_engine_create(uint8_t metric, uint32_t dims, int device_id, wax_hip_engine** out);
/* The same engine over several GPUs of one node, in ONE process (the reference has no multi-device path):
 * the handle owns one single-device engine ("shard") per listed HIP ordinal (duplicates allowed: two shards on one GPU, for
 * tests). Rows are kept in contiguous blocks — shard g holds global rows [base_g, base_g + count_g), base_g = the rows before
 * it — so the concatenation of the shards is the insertion order of ONE engine: every entry point of this header that takes
 * a handle works on it with identical results (same tie rule, same serialize bytes). A shard is full at ceil(N / n_devices)
 * rows after wax_hip_reserve(N) (or the first batch); when every shard is full the block size doubles (peer-copy rebalance).
 * search: per shard on its own stream, query upload + fused scan + per-shard top-k, then the k hits (16 k bytes per shard)
 * are peer-copied to the first device and merged there by key (tuning "exchange" = 1: one ncclAllGather per query on a
 * single-process RCCL communicator instead). Batched search: every shard answers the batch on its rows through the
 * single-device submit / collect pair (one host thread drives all shards: nothing blocks between them, no thread and no
 * allocation per call), the first device merges per query; the device-resident forms (wax_hip_search_batch_hits_device,
 * _submit_device / _collect_device) work on the handle too — queries and hits then live in the FIRST device's HBM, the query
 * block is peer-copied to the other shards and only nq x k hits per shard come back. An unavailable ordinal fails with
 * WAX_HIP_ERR_NO_DEVICE. Single-device-only entry points (wax_hip_set_row_base, wax_hip_search_shard_device, the two
 * wax_hip_time_* probes) return WAX_HIP_ERR_INVALID_ARGUMENT on such a handle. */
int wax_hip_engine_create_sharded(uint8_t metric, uint32_t dims, const int* device_ids, int n_devices, wax_hip_engine** out);
/* 1 for a single-device engine; shard -> (device ordinal, first global row, rows). */
int wax_hip_shard_count(const wax_hip_engine* e);
int wax_hip_shard_info(const wax_hip_engine* e, int shard, int* out_device, uint64_t* out_row_base, uint64_t* out_rows);
void wax_hip_engine_destroy(wax_hip_engine* e);

/* VectorSearchEngine.dimensions (VectorSearchEngine.swift:11) */
uint32_t wax_hip_dimensions(const wax_hip_engine* e);
/* vectorCount (MetalVectorEngine.swift:51) */
uint64_t wax_hip_count(const wax_hip_engine* e);
uint8_t wax_hip_metric_of(const wax_hip_engine* e);
int wax_hip_device_of(const wax_hip_engine* e);

/* ---- store mutation (exclusive lock) ------------------------------------ */

/* add(frameId:vector:) — upsert by frame id (MetalVectorEngine.swift:330-357). */
int wax_hip_add(wax_hip_engine* e, uint64_t frame_id, const float* vector, uint32_t dims);
/* addBatch(frameIds:vectors:) (MetalVectorEngine.swift:359-402); rows is row-major n x dims.
 * addBatchStreaming (:404-421) is the same call made in chunks by the caller. */
int wax_hip_add_batch(wax_hip_engine* e, const uint64_t* frame_ids, const float* rows, uint64_t n, uint32_t dims);
/* Same, but `rows` is a DEVICE pointer on the engine's device (embeddings that
 * were produced in HBM never bounce through the host). frame_ids stays a host
 * pointer. All ids must be new (append-only fast path); WAX_HIP_ERR_INVALID_ARGUMENT otherwise. */
int wax_hip_add_batch_device(wax_hip_engine* e, const uint64_t* frame_ids, const float* d_rows, uint64_t n, uint32_t dims);
/* Pending-embedding replay (UnifiedSearchEngineCache.applyPendingEmbeddingsIfNeeded, UnifiedSearchEngineCache.swift:252-283;
 * MetalVectorEngine.load, MetalVectorEngine.swift:318-328): `payloads` is `len` bytes of WAL putEmbedding entry
 * payloads laid back to back exactly as WALEntryCodec.encode writes them (WALEntryCodec.swift:39-54):
 * u8 opcode 0x04, u64 frameId LE, u32 dimension LE, dimension x f32 LE. The stream is validated as a whole
 * (decode rules of WALEntryCodec.swift:104-129: unknown opcode, dimension > 1 000 000, truncated record ->
 * WAX_HIP_ERR_BAD_SEGMENT; dimension != engine dims -> WAX_HIP_ERR_DIM_MISMATCH) and then applied in order
 * as ONE addBatch (later records of the same frame overwrite earlier ones), so a bad stream changes nothing.
 * *out_applied (may be NULL) receives the number of records. */
int wax_hip_apply_put_embeddings(wax_hip_engine* e, const uint8_t* payloads, uint64_t len, uint64_t* out_applied);
/* remove(frameId:) — order-preserving delete, absent id is a no-op (MetalVectorEngine.swift:423-444). */
int wax_hip_remove(wax_hip_engine* e, uint64_t frame_id);
/* remove(frameId:) for many ids at once (the loop of VectorSearchSession.swift:188-192 as one call). The engine ends in exactly
 * the state that calling wax_hip_remove(e, frame_ids[i]) for i = 0 .. n-1 would leave: absent ids are ignored, an id listed twice
 * counts once, the surviving rows keep their order. *out_removed (may be NULL) = rows actually removed. n == 0 is a no-op.
 * One exclusive-lock acquisition and ONE order-preserving compaction pass: every surviving row behind the first removed one moves
 * down once, by the number of removed rows in front of it (store, frame ids, and the bf16 mirror with its norms, which is
 * compacted, not converted again); the host's id vector and id map are fixed in one pass each. Extra device memory: the 64 MB
 * bounce buffer and 4 bytes per removed row, whatever the store's size. Arguments, the row list's upload and the scratch
 * allocation are checked before the first row moves. A store that holds one frame id in several rows (only wax_hip_deserialize
 * can produce one; detected exactly, by the id map holding fewer ids than the store has rows) is answered by the per-id loop
 * instead — same result, n passes. On a sharded handle every shard that owns listed ids compacts once. */
int wax_hip_remove_batch(wax_hip_engine* e, const uint64_t* frame_ids, uint64_t n, uint64_t* out_removed);
/* reserveIfNeeded(for:) (MetalVectorEngine.swift:857-871): capacity doubling from 64, cap UInt32.max rows. */
int wax_hip_reserve(wax_hip_engine* e, uint64_t rows);

/* ---- search (shared lock, re-entrant) ----------------------------------- */

/* clampTopK (MetalVectorEngine.swift:842-846): the number of entries a result array needs so that no
 * result is ever truncated, independent of the engine's current row count. */
uint32_t wax_hip_result_capacity(int32_t top_k);

/* VectorSearchEngine.search(vector:topK:) (VectorSearchEngine.swift:13;
 * MetalVectorEngine.swift:446-627). Blocking. out_ids/out_scores hold out_capacity
 * entries; *out_count receives how many were written = min(clamp(top_k,1,10000), count,
 * out_capacity) minus dropped non-finite entries (best first: descending score == ascending
 * distance, ties by ascending row; a capacity below the result count keeps the best ones).
 * Empty engine => OK with *out_count = 0 (:448). */
int wax_hip_search(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k,
                   uint64_t* out_ids, float* out_scores, uint32_t out_capacity, uint32_t* out_count);

/* Pipelined form of the same call: submit enqueues H2D + kernels + D2H on one
 * of the engine's scratch slots and returns immediately with a ticket;
 * collect blocks on that slot and fills the outputs exactly like
 * wax_hip_search. Tickets must be collected exactly once, in any order (also from another
 * thread). A thread that already holds tickets never waits for a scratch slot (it gets a fresh one,
 * up to 256 outstanding), so pipelining callers cannot deadlock each other. A ticket holds the engine's
 * shared lock until it is collected: a mutation (add / remove / reserve / deserialize / set_row_base)
 * called by a thread that still holds uncollected tickets would wait for itself forever, so it fails
 * with WAX_HIP_ERR_INVALID_ARGUMENT ("collect outstanding search tickets first") instead. */
int wax_hip_search_submit(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, uint64_t* out_ticket);
int wax_hip_search_collect(wax_hip_engine* e, uint64_t ticket,
                           uint64_t* out_ids, float* out_scores, uint32_t out_capacity, uint32_t* out_count);

/* nq queries, row-major nq x dims. out_ids/out_scores are nq rows of out_stride entries (query q's
 * results start at q * out_stride; at most out_stride are written per query); out_counts[nq]. */
int wax_hip_search_batch(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k,
                         uint64_t* out_ids, float* out_scores, uint32_t out_stride, uint32_t* out_counts);

/* Same search, but the raw ranked candidates are returned: out_hits is nq rows of out_stride wax_hip_hit
 * (ascending key, every row padded to out_stride with key = INT64_MAX). This is what a row-sharded deployment exchanges between ranks and
 * merges by key (exact tie order by GLOBAL row, see wax_hip_set_row_base). Large batches run Q x D^T as a
 * bf16 MFMA GEMM with an exact f32 re-score; results are identical to nq calls of wax_hip_search. */
int wax_hip_search_batch_hits(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k,
                              wax_hip_hit* out_hits, uint32_t out_stride, uint32_t* out_counts);

/* Device-resident form of the same search: d_queries is nq x dims f32 in HBM on the engine's device (embeddings that
 * were produced on the GPU never bounce through the host), d_out_hits receives nq rows of out_stride hits in HBM
 * (ascending key, padded). Blocking. `stream` (a hipStream_t, NULL = the null stream) is the stream whose earlier
 * work produced d_queries; the library orders its own work behind it, and on return all results are complete.
 * Inside, the batch runs without a host round trip (certificate flags come back once, at the end); uncertified
 * queries are re-run on the exact path in place. This is the entry point the batched BASELINE configs are timed on
 * (inputs resident in HBM), and what a row-sharded deployment feeds to its RCCL all-gather. */
int wax_hip_search_batch_hits_device(wax_hip_engine* e, const float* d_queries, uint32_t nq, uint32_t dims, int32_t top_k,
                                     wax_hip_hit* d_out_hits, uint32_t out_stride, void* stream);

/* Pipelined form (the batched counterpart of wax_hip_search_submit / _collect, i.e. of the command-buffer overlap the
 * reference gets from MTLCommandQueue): submit enqueues the whole batch on one of the engine's batch workspaces, ordered
 * behind `stream`, and returns at once with a ticket; collect waits for it, re-runs uncertified queries on the exact path
 * in place, and reports how many that were (out_fallbacks may be NULL). With two or more tickets in flight the next batch's
 * launches and the host's wake-up hide under the running batch. d_queries / d_out_hits must stay valid and untouched until
 * collect. At most "batch_workspaces" (default 4) tickets per engine; a ticket holds the engine's read lock like a
 * single-query ticket (writers are refused with WAX_HIP_ERR_INVALID_ARGUMENT while the calling thread holds one). */
int wax_hip_search_batch_submit_device(wax_hip_engine* e, const float* d_queries, uint32_t nq, uint32_t dims, int32_t top_k,
                                       wax_hip_hit* d_out_hits, uint32_t out_stride, void* stream, uint64_t* out_ticket);
int wax_hip_search_batch_collect_device(wax_hip_engine* e, uint64_t ticket, uint32_t* out_fallbacks);

/* ---- rank fusion on the device ----
 *
 * Weighted reciprocal-rank fusion of ranked frame-id lists for nq queries at once: HybridSearch.rrfFusion(lists:k:)
 * (HybridSearch.swift:25-52) == UnifiedSearch.rrfFusionResults (UnifiedSearch.swift:590-699) without the diagnostics.
 * Lanes are taken in order; a lane with weight <= 0 is skipped; the entry at 0-based position p of a lane adds
 * weight / Float(max(0, k) + p + 1) to its frame's f32 score (lane order, then position order: scores are bit-identical
 * to the Swift loop); bestRank = the smallest p + 1 over the lanes that name the frame; sources = bit l set when lane l
 * names it. Per query the output row holds every frame seen, best first by (score desc, bestRank asc, frameId asc),
 * truncated / padded (frame id UInt64.max, score 0) to out_stride; d_out_counts[q] = real entries.
 *
 * Lane l of query q: entry p is d_ids[(q * stride + p) * pitch] (pitch 1 = a plain id array; pitch 2 with d_ids pointing at
 * the frame_id field = a wax_hip_hit array straight out of wax_hip_search_batch_hits_device), d_counts[q] entries (NULL:
 * stride entries); entries equal to UInt64.max (the padding of a hit list) are skipped. All pointers are device memory on
 * the current device; the call enqueues on `stream` and returns. Limits: n_lanes <= 8, sum of the strides <= 4096,
 * k <= 2^30. d_out_best_rank / d_out_sources / d_out_counts may be NULL. */
#define WAX_HIP_RRF_MAX_LANES 8
#define WAX_HIP_RRF_MAX_ENTRIES 4096
typedef struct wax_hip_rrf_lane {
    const uint64_t* d_ids;
    const uint32_t* d_counts;
    uint32_t stride;
    uint32_t pitch;
    float weight;
} wax_hip_rrf_lane;
int wax_hip_rrf_fuse_batch_device(const wax_hip_rrf_lane* lanes, uint32_t n_lanes, uint32_t nq, int32_t k,
                                  uint64_t* d_out_ids, float* d_out_scores, uint32_t* d_out_best_rank,
                                  uint32_t* d_out_sources, uint32_t out_stride, uint32_t* d_out_counts, void* stream);
/* One query from host memory (what UnifiedSearch holds when the text lane comes from FTS5): uploads the lists, fuses on
 * `device_id` (-1 = current), downloads. lists[l] has list_counts[l] ids; at most out_capacity results are written. */
int wax_hip_rrf_fuse(const float* weights, const uint64_t* const* lists, const uint32_t* list_counts, uint32_t n_lists,
                     int32_t k, int device_id, uint64_t* out_ids, float* out_scores, uint32_t* out_best_rank,
                     uint32_t* out_sources, uint32_t out_capacity, uint32_t* out_count);

/* ---- sharded search: per-shard top-k left in HBM for the RCCL exchange ---- */

/* Declares that this engine holds rows [row_base, row_base+count) of a corpus
 * that is row-sharded over several engines/GPUs. row_base is
 * folded into wax_hip_hit.key so ties break by GLOBAL row on every shard count. */
int wax_hip_set_row_base(wax_hip_engine* e, uint64_t row_base);
/* Scan this shard for one query and write exactly kpad = clamp(top_k) hits,
 * sorted ascending by key, to the DEVICE buffer d_out_hits (entries past the
 * shard's own count are padded with key = INT64_MAX, frame_id = UINT64_MAX).
 * Work is enqueued on `stream` (a hipStream_t; NULL = the null stream) and NOT
 * synchronised: the caller all-gathers d_out_hits over RCCL on the same stream
 * order and then calls wax_hip_merge_hits_device. top_k must be <= 192 here. */
int wax_hip_search_shard_device(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k,
                                wax_hip_hit* d_out_hits, void* stream);
/* Stateless G*k -> k merge of gathered shard results on the current device:
 * d_out receives the k smallest keys of d_in[0..n), ascending. n <= 16384. */
int wax_hip_merge_hits_device(const wax_hip_hit* d_in, uint32_t n, uint32_t k, wax_hip_hit* d_out, void* stream);
/* Batched form for the sharded batched path (BASELINE config 5): d_in = [n_shards][nq][k_in] hits (the all-gather
 * of every shard's wax_hip_search_batch_hits result, copied to the device), d_out = [nq][k]: per query the k
 * smallest keys, ascending. One workgroup per query. n_shards * k_in <= 16384, k <= 192. */
int wax_hip_merge_batch_hits_device(const wax_hip_hit* d_in, uint32_t n_shards, uint32_t nq, uint32_t k_in, uint32_t k,
                                    wax_hip_hit* d_out, void* stream);
/* Host-side tail of search (MetalVectorEngine.swift:592-611 + VectorMetric.swift:32-43):
 * drop padded / non-finite entries, distance -> score, emit (frameId, score); out arrays hold n entries. */
int wax_hip_hits_to_results(uint8_t metric, const wax_hip_hit* hits, uint32_t n,
                            uint64_t* out_ids, float* out_scores, uint32_t* out_count);

/* ---- filtered search (the vector lane's candidate filters, applied on the device) -------- *
 * UnifiedSearch applies FrameFilter.frameIds (an allow-list) and SearchRequest.minScore to the vector lane's
 * candidates AFTER the engine returned them (passesFrameFilter, UnifiedSearch.swift:1241-1258), so it asks the engine
 * for candidateLimit = max(topK, min(3 topK, 1000)) results (:1195-1200) and can still come back short when the
 * allowed frames rank deeper (the reference test only covers a 4-document corpus,
 * UnifiedSearchTests.swift:133-158). Here the allow-list is a PRE-filter: only the allowed rows are scored
 * (cost ~ allowed rows, not corpus rows) and the top_k of THEM comes back, then results with score < min_score are
 * dropped. has_allow = 0: no allow-list (allow_frame_ids ignored); has_allow = 1 with n_allow = 0: nothing is
 * allowed. Ids not in the engine are ignored. has_min_score = 0: no score cut. Distances are bit-identical to
 * wax_hip_search's for the same rows. */
int wax_hip_search_filtered(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k,
                            int has_allow, const uint64_t* allow_frame_ids, uint64_t n_allow,
                            int has_min_score, float min_score,
                            uint64_t* out_ids, float* out_scores, uint32_t out_capacity, uint32_t* out_count);

/* Batched filtered search: nq queries (row-major nq x dims), each with its own allow-list and score cut.
 * Allow-lists: allow_begin and allow_len both NULL = no query has a list. Otherwise query q's list is
 * allow_frame_ids[allow_begin[q] .. allow_begin[q] + allow_len[q]); allow_len[q] == WAX_HIP_NO_ALLOW_LIST = no list for q;
 * length 0 = nothing allowed. Ranges may overlap; queries with the same (begin, len) share one list, which is resolved once and
 * scored for all of them in one pass. A range that leaves [0, n_allow_ids) is refused (WAX_HIP_ERR_INVALID_ARGUMENT). Ids not in
 * the engine are ignored; duplicate ids count once. min_scores NULL = no cut, otherwise query q drops results with
 * score < min_scores[q] (NaN: no cut). Outputs as wax_hip_search_batch: row q at q * out_stride, out_counts[q] results.
 * Row q equals wax_hip_search_filtered for that query, list and cut with out_capacity = out_stride, bit for bit; a query with
 * neither list nor cut gets its wax_hip_search_batch row. The queries with a list are answered under one shared-lock
 * acquisition (one snapshot of the store); those without one run first as one sub-batch of the unfiltered batched search.
 * Up to FUSED_MAX_K (192) results and the specialised dimensions (64, 128, 256, 384, 512, 768, 1024, 1536): every list is
 * sorted into a compact row list on the device and one gather launch scores all lists, with one synchronisation per call.
 * Otherwise, and with "filter_batch" 0 or "force_general" set, each listed query takes the single-query filtered path. */
#define WAX_HIP_NO_ALLOW_LIST UINT64_MAX
int wax_hip_search_batch_filtered(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k,
                                  const uint64_t* allow_frame_ids, uint64_t n_allow_ids,
                                  const uint64_t* allow_begin, const uint64_t* allow_len,
                                  const float* min_scores,
                                  uint64_t* out_ids, float* out_scores, uint32_t out_stride, uint32_t* out_counts);

/* One query each against MANY stores of one device, in one pass: pair i is (engines[i], queries + i * dims). It stands in for
 * VectorSearchEngine.search(vector:topK:) called once per store by a host that serves one store per user or agent: a vec segment is
 * capped at 256 MiB (Constants.swift:49: at most 174 762 rows at 384-d), so one device holds hundreds of stores and its traffic is one
 * query each against many of them — per store a call of its own pays its own upload, launch, completion and download.
 * Row i of the outputs (at i * out_stride, out_counts[i] results) equals wax_hip_search(engines[i], query i, dims, top_k, ...) with
 * out_capacity = out_stride: ids and scores bit for bit, ties in ascending row order, the same top_k clamp. An engine may be listed
 * any number of times (its queries share passes over its store, up to 16 per pass); an empty engine gives count 0; n == 0 returns
 * WAX_HIP_OK and touches nothing. Refused before any lock is taken or anything is launched, outputs untouched, the pair's index in
 * wax_hip_last_error(): a NULL entry, a sharded handle, engines on different devices or of different metrics
 * (WAX_HIP_ERR_INVALID_ARGUMENT); an engine whose dimensions != dims (WAX_HIP_ERR_DIM_MISMATCH, wax_hip_search's message).
 * One snapshot: the shared locks of all distinct engines are held together for the call (taken in ascending address order of the
 * handles; re-entrant for a thread that holds tickets), and rows staged by wax_hip_add just before the call are seen.
 * Pairs whose engine holds at most "search_many_max_rows" rows, at the specialised dimensions and top_k <= 192 (<= 60 from 512-d
 * up), are scored by ONE launch for all their stores, merged by one more, downloaded and synchronised once; every
 * other pair, and every pair of an engine with "search_many" 0 or "force_general" set, runs the single-query search under the same
 * locks. */
int wax_hip_search_many(wax_hip_engine* const* engines, const float* queries, uint32_t n, uint32_t dims, int32_t top_k,
                        uint64_t* out_ids, float* out_scores, uint32_t out_stride, uint32_t* out_counts);

/* ---- per-row attributes and the predicate search ------------------------------------------------------------ *
 * passesFrameFilter (UnifiedSearch.swift:1241-1258) also drops vector-lane candidates by per-frame metadata: request.timeRange
 * against FrameMeta.timestamp (TimeRange.contains, SearchRequest.swift:91-105), status == .deleted, supersededBy != nil and
 * kind == "surrogate" — the last three excluded by the default FrameFilter(). Two optional per-row columns carry that metadata
 * beside the store: int64 timestamp and uint32 flags. A store on which they were never set behaves as if every row were (0, 0)
 * and allocates nothing for them. An appended row gets (0, 0); an upsert keeps its row's attributes; removals take the row's
 * entry with them; reserve and growth keep them; wax_hip_deserialize drops them all (MV2V has no field for them, and
 * wax_hip_serialize is unchanged). The host holds the authoritative copy; the device mirror is brought up to date by the first
 * predicate search after a change (appended rows only, or everything from the lowest changed row). */
#define WAX_HIP_FLAG_DELETED    0x1u   /* FrameMeta.status == .deleted (UnifiedSearch.swift:1249) */
#define WAX_HIP_FLAG_SUPERSEDED 0x2u   /* FrameMeta.supersededBy != nil (UnifiedSearch.swift:1250) */
#define WAX_HIP_FLAG_SURROGATE  0x4u   /* FrameMeta.kind == "surrogate" (UnifiedSearch.swift:1251-1254) */
#define WAX_HIP_FLAG_USER_SHIFT 8      /* bits 8..31 are the caller's */
/* FrameMeta.timestamp / status / supersededBy / kind of the listed frames (the values UnifiedSearch.swift:1245-1256 reads).
 * timestamps NULL = leave every timestamp as it is, flags NULL likewise. Ids the engine does not hold are skipped; an id
 * listed twice takes its last entry. *out_applied (may be NULL) = entries that named a held frame. A writer: exclusive lock,
 * refused while the calling thread holds uncollected search tickets. */
int wax_hip_set_attributes(wax_hip_engine* e, const uint64_t* frame_ids, const int64_t* timestamps, const uint32_t* flags,
                           uint64_t n, uint64_t* out_applied);
/* The same columns read back (the FrameMeta fields above). out_found[i] = 1 and the row's values, or 0 and (0, 0) for an id
 * the engine does not hold. Any of the three output arrays may be NULL. */
int wax_hip_get_attributes(wax_hip_engine* e, const uint64_t* frame_ids, uint64_t n, int64_t* out_timestamps,
                           uint32_t* out_flags, uint8_t* out_found);
/* SearchRequest.timeRange (TimeRange.contains, SearchRequest.swift:91-105: after inclusive, before exclusive) and the flag
 * exclusions of FrameFilter (UnifiedSearch.swift:1249-1254). A row passes iff !(has_after && ts < after) &&
 * !(has_before && ts >= before) && (flags & deny_flags) == 0. */
typedef struct wax_hip_row_predicate {
    int32_t has_after;
    int64_t after;
    int32_t has_before;
    int64_t before;
    uint32_t deny_flags;
} wax_hip_row_predicate;
/* passesFrameFilter (UnifiedSearch.swift:1241-1258) as a PRE-filter: wax_hip_search_filtered's arguments plus the row predicate.
 * Returns the best top_k among the rows that pass the predicate AND the allow-list (if given), best first, ties in ascending row
 * order, fewer if fewer pass; then results with score < min_score are dropped. Distances are bit-identical to wax_hip_search's
 * for the same rows. pred NULL, or one with no bound and no deny bit, is wax_hip_search_filtered. The predicate is evaluated on
 * the device into a row bitmap; then either the passing rows are gathered and scored (few pass, top_k > 192, dims outside the
 * specialised set, "force_general") or the f32 scan runs with the bitmap, skipping the loads of chunks without a passing row
 * ("predicate_route", "predicate_scan_min_permille"). On a store above 2 GiB of f32 rows that scan streams the bf16
 * mirror under the same bitmap instead, re-scores its 64 best passing rows in f32 and returns them only under the mirror scan's
 * certificate — the same answer bit for bit; without the certificate the f32 scan answers ("predicate_mirror"). */
int wax_hip_search_predicate(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k,
                             int has_allow, const uint64_t* allow_frame_ids, uint64_t n_allow,
                             int has_min_score, float min_score, const wax_hip_row_predicate* pred,
                             uint64_t* out_ids, float* out_scores, uint32_t out_capacity, uint32_t* out_count);
/* passesFrameFilter (UnifiedSearch.swift:1241-1258) as a PRE-filter on a TICKET: wax_hip_search_predicate without an allow-list, in
 * the pipelined form of wax_hip_search_submit. The ticket is collected by wax_hip_search_collect (one ticket namespace) and what it
 * returns equals, bit for bit, wax_hip_search_predicate(e, query, dims, top_k, 0, NULL, 0, has_min_score, min_score, pred, ...):
 * ids, scores, count, ties in ascending row order. Like every ticket it holds the engine's shared lock until it is collected; a
 * writer on a thread that holds one is refused. Routing at submit ("Predicate tickets"): NULL arguments and a dimension
 * mismatch are refused as wax_hip_search_predicate refuses them; a predicate with no bound and no deny bit makes the call
 * wax_hip_search_submit, with the cut applied at collect; an empty engine gives an empty ticket; a store on which attributes were
 * never set decides the predicate on the host (an ordinary ticket, or one of count 0 without device work). Otherwise the ticket
 * RIDES a pass over the 8-bit code mirror under a row bitmap — on a single-device engine, where "predicate_mirror" and "mirror_bits"
 * (and its breaker) admit top_k, and one of the engine's four bitmap entries is free or already holds this predicate for the store
 * as it is — parked, filled and launched like an unfiltered mirror ticket ("mirror_share", "mirror_fill") and in the same sets: a
 * set with a masked member runs the masked form of the pass, its unfiltered members beside it. A bitmap is built once per
 * (predicate, store state) on the launching stream, without a host synchronisation. Every other ticket is DEFERRED: its collect runs
 * the blocking call's body under the lock the ticket holds (a sharded handle, L2, other dimensions, top_k > 16, "predicate_mirror" 0,
 * "force_general", no free bitmap entry, a bitmap known to hold 64 rows or fewer). A ticket that rode without its certificate is
 * answered by that body as well. */
int wax_hip_search_predicate_submit(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k, int has_min_score,
                                    float min_score, const wax_hip_row_predicate* pred, uint64_t* out_ticket);
/* What became of the predicate tickets of this engine, in the way of wax_hip_mirror8_snapshot (a read-out, no tuning key): submitted
 * (non-empty predicates), rode (launched in a masked pass), masked_passes, certified, fallbacks (rode, answered by the blocking
 * body), deferred, host_decided, bitmap_builds, bitmap_hits (tickets that found their bitmap in an entry). A sharded handle reports
 * its own `submitted` and `deferred`; the other fields are 0 there. */
typedef struct wax_hip_predicate_ticket_stats_t {
    uint64_t submitted, rode, masked_passes, certified, fallbacks, deferred, host_decided, bitmap_builds, bitmap_hits;
} wax_hip_predicate_ticket_stats_t;
int wax_hip_predicate_ticket_stats(wax_hip_engine* e, wax_hip_predicate_ticket_stats_t* out);
/* wax_hip_search_many with a row predicate and a score cut PER PAIR — what a host with one store per user needs, since no Wax query
 * is unfiltered (the default FrameFilter() already drops deleted, superseded and surrogate frames). preds: n entries, or NULL = no
 * pair has one; min_scores: n entries, or NULL = no cut (NaN = no cut for that pair). Row i equals, bit for bit,
 * wax_hip_search_predicate(engines[i], query i, dims, top_k, 0, NULL, 0, min_scores != NULL, min_scores[i], &preds[i], ...) with
 * out_capacity = out_stride: its ids, scores and count, ties in ascending row order, fewer results when fewer rows pass. A pair
 * whose predicate has no bound and no deny bit is an ordinary wax_hip_search_many pair, and with preds == NULL and
 * min_scores == NULL the call IS wax_hip_search_many (one body serves both). Refusals (their order, their messages, the pair's
 * index, outputs untouched), the snapshot (shared locks of all distinct engines in ascending address order, staged rows flushed)
 * and the routes are wax_hip_search_many's; n == 0 returns WAX_HIP_OK and touches nothing. Allow-lists per pair are NOT part of
 * this call (wax_hip_search_predicate / wax_hip_search_batch_filtered take them, one store at a time).
 * Pooled pairs (wax_hip_search_many's rule) of one engine share passes by predicate: the pairs with the same predicate — an unused
 * bound's value does not count — form groups of up to 16, so queries that share a predicate share a pass. The predicates become row
 * bitmaps in ONE launch ahead of the pooled scan, which then offers only rows whose bit is set; there is no host round trip for
 * pass counts, and still one download and one synchronisation per call. A store on which attributes were never set reads as (0, 0)
 * in every row: its predicates are decided on the host (the pair is unmasked, or its count is 0 without device work). Every other
 * pair runs the single-query predicate search under the locks the call holds. The cut is applied on the host, whatever the route. */
int wax_hip_search_many_predicate(wax_hip_engine* const* engines, const float* queries, uint32_t n, uint32_t dims, int32_t top_k,
                                  const wax_hip_row_predicate* preds, const float* min_scores,
                                  uint64_t* out_ids, float* out_scores, uint32_t out_stride, uint32_t* out_counts);
/* wax_hip_search_batch_filtered with a row predicate PER QUERY: nq queries against ONE store, each with its own allow-list, score cut
 * and predicate. preds: nq entries, or NULL = no query has one; every other argument means what it means in
 * wax_hip_search_batch_filtered. Row q equals, bit for bit (ids, scores, count, ties in ascending row order),
 * wax_hip_search_predicate(e, query q, dims, top_k, has list q, list q, len q, min_scores != NULL, min_scores[q], &preds[q], ...)
 * with out_capacity = out_stride. A query whose predicate has no bound and no deny bit is a wax_hip_search_batch_filtered query, and
 * with preds == NULL the call IS wax_hip_search_batch_filtered (one body serves both): the same launches, the same counters.
 * Refusals (their order, their messages, outputs untouched), the sharded dispatch and the snapshot are that call's.
 * Queries with the same (begin, len | no list, predicate) — an unused bound's value does not count — share an ENTRY and its groups
 * of up to 16 queries. Every entry becomes a compact ascending row list with a device-side count: a list of at most 16 384 ids by the
 * LDS sort, rows that fail the predicate dropped before the sort; a longer list by the single-query route's launches (probe,
 * attribute mask ANDed into the bitmap, compaction); an entry without a list straight from the attribute columns, ALL such entries of
 * the call in three launches. One gather launch then scores every entry, one merge attaches ids: one download, one synchronisation,
 * no host round trip for pass counts. Every group of 16 queries re-reads its entry's passing rows, so a predicate that
 * passes most of a large store costs about nq / 16 passes over it. A store on which attributes were never set reads (0, 0) in every
 * row: its predicates are decided on the host (the query loses its predicate, or its count is 0 without device work). Entries with a
 * predicate are admitted in order of their first query while their upper bounds (min(len, count); count without a list) fit
 * "predicate_batch_rows" row slots; the queries of the rest, and every query where wax_hip_search_batch_filtered itself falls back
 * (top_k > 192, other dimensions, "filter_batch" 0, "force_general"), take the single-query predicate search under the lock held. */
int wax_hip_search_batch_predicate(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k,
                                   const uint64_t* allow_frame_ids, uint64_t n_allow_ids,
                                   const uint64_t* allow_begin, const uint64_t* allow_len,
                                   const float* min_scores, const wax_hip_row_predicate* preds,
                                   uint64_t* out_ids, float* out_scores, uint32_t out_stride, uint32_t* out_counts);

/* ---- the timeline lane ------------------------------------------------------------------------------------------ *
 * Wax.timeline(TimelineQuery) (TimelineQuery.swift:38-53) is the third ranked id list UnifiedSearch fuses (UnifiedSearch.swift:181-194,
 * with limit = max(candidateLimit, timelineFallbackLimit): 30 to 1 000): the `limit` newest (or oldest) frames that pass after /
 * before and the deleted / superseded exclusions. Here it is selected on the device from the attribute columns above: a row passes
 * under wax_hip_row_predicate's rule (a store, or a row, without attributes is (0, 0)), and the answer is the first `limit` passing
 * rows by (timestamp ascending, frame id ascending) for chronological order, (timestamp descending, frame id ascending) for
 * newest_first != 0. Ties go by ascending FRAME ID, compared unsigned, not by row: toc.frames is indexed by frame id and Swift's sort
 * is stable, so that is what the reference returns in both orders, and it makes the answer independent of the store's mutation
 * history and of sharding. includeDeleted / includeSuperseded map to deny_flags as in wax_hip_search_predicate. The reference drops
 * surrogates AFTER the prefix; WAX_HIP_FLAG_SURROGATE in deny_flags makes that a PRE-filter here: the limit newest of the frames that
 * are not surrogates, never fewer because surrogates crowded the prefix. */
#define WAX_HIP_TIMELINE_MAX_LIMIT 4096   /* = WAX_HIP_RRF_MAX_ENTRIES: a longer lane cannot be fused */
/* Blocking. A reader: shared lock, rows staged by wax_hip_add are seen, re-entrant for a thread that holds tickets. Writes
 * min(passing rows, limit, out_capacity) ids (and their timestamps: out_timestamps may be NULL) and that number to *out_count.
 * limit <= 0: count 0, no device is touched (TimelineQuery.swift:51). pred NULL: every row passes. An empty engine gives count 0.
 * A sharded handle runs every shard and merges on the host by the same pair order. Refused with WAX_HIP_ERR_INVALID_ARGUMENT, the
 * outputs untouched: a NULL engine, a NULL out_count, NULL out_ids with out_capacity != 0, limit > WAX_HIP_TIMELINE_MAX_LIMIT. */
int wax_hip_timeline(wax_hip_engine* e, int32_t limit, int newest_first, const wax_hip_row_predicate* pred,
                     uint64_t* out_ids, int64_t* out_timestamps, uint32_t out_capacity, uint32_t* out_count);
/* The same answer left in HBM: exactly `limit` ids to d_out_ids, entries past the answer padded with UINT64_MAX, and the real count
 * to *d_out_count. Enqueued on `stream` and NOT synchronised, under the contract of wax_hip_search_shard_device — the result is a lane
 * for wax_hip_rrf_fuse_batch_device with stride = limit, pitch = 1 on the same stream. The attribute columns are brought up to date
 * as the blocking predicate search does it, on a stream of the engine's, and `stream` waits for that by an event. limit <= 0 writes
 * count 0 only. A sharded handle is refused. */
int wax_hip_timeline_device(wax_hip_engine* e, int32_t limit, int newest_first, const wax_hip_row_predicate* pred,
                            uint64_t* d_out_ids, uint32_t* d_out_count, void* stream);

/* ---- grouped search: best parents by best member, members per parent ---------------------------------------------- *
 * What PhotoRAGOrchestrator.recall (PhotoRAGOrchestrator.swift:264-317) and VideoRAGOrchestrator.recall
 * (VideoRAGOrchestrator.swift:252, 273-417) do with the vector lane's answer: collapse the hits by `meta.parentId ?? meta.id`, score a
 * root by its best member (`entry.score = max(entry.score, result.score)`), order roots by (score descending, rootId ascending), keep
 * resultLimit roots (default 12) and, for video, segmentLimitPerVideo (default 3) best segments per root. The reference over-fetches
 * rows (topK = max(400, resultLimit * segmentLimitPerVideo * 8); 200 for photos) and collapses on the host, which returns too few or
 * the wrong roots when one root owns the over-fetched prefix. Here one pass over the store answers exactly.
 *
 * A third optional per-row column carries a uint64 parent id beside the two attribute columns above, under their lifecycle word for
 * word: a store on which parents were never set allocates nothing and every row is its own root; an appended row gets
 * WAX_HIP_NO_PARENT; an upsert keeps its row's parent; removals take the row's entry with them; reserve and growth keep the column; a
 * move between shards carries it; wax_hip_deserialize drops it (MV2V has no field for it, and wax_hip_serialize is unchanged). The
 * host copy is authoritative; the device copy is brought up to date by the first grouped search after a change. A row's ROOT is its
 * parent, or its own frame id where the parent is WAX_HIP_NO_PARENT (`meta.parentId ?? meta.id`, PhotoRAGOrchestrator.swift:282,
 * VideoRAGOrchestrator.swift:314). A root need not be a frame the engine holds: roots often have no embedding. */
#define WAX_HIP_NO_PARENT UINT64_MAX
/* FrameMeta.parentId of the listed frames (the value PhotoRAGOrchestrator.swift:282 / VideoRAGOrchestrator.swift:314 read). Writer and
 * reader exactly as wax_hip_set_attributes / wax_hip_get_attributes are: ids the engine does not hold are skipped, an id listed twice
 * takes its last entry, *out_applied (may be NULL) = entries that named a held frame, a thread that holds uncollected search tickets is
 * refused, a sharded handle routes every id to the shard that owns it. out_found[i] = 1 and the row's parent, or 0 and
 * WAX_HIP_NO_PARENT for an id the engine does not hold; either output array may be NULL. */
int wax_hip_set_parents(wax_hip_engine* e, const uint64_t* frame_ids, const uint64_t* parent_ids, uint64_t n, uint64_t* out_applied);
int wax_hip_get_parents(wax_hip_engine* e, const uint64_t* frame_ids, uint64_t n, uint64_t* out_parents, uint8_t* out_found);
#define WAX_HIP_GROUP_MAX_LIMIT   1024
#define WAX_HIP_GROUP_MAX_MEMBERS 8
/* The `limit` best roots and, per root, its `per_group` best rows (PhotoRAGOrchestrator.swift:264-317 with per_group 1;
 * VideoRAGOrchestrator.swift:273-417 with per_group = segmentLimitPerVideo). Blocking; a reader: shared lock, rows staged by
 * wax_hip_add are seen, re-entrant for a thread that holds tickets. The answer, exactly:
 *  1. Only rows that pass pred take part (wax_hip_row_predicate's rule; NULL = every row). A row whose distance is not finite takes
 *     no part, as in wax_hip_search.
 *  2. A group is the set of participating rows with one root; its distance is the smallest distance among its rows — the bits
 *     wax_hip_search gives those rows.
 *  3. Groups are ordered by (distance ascending, root id ascending as unsigned): the tie goes by ROOT ID, not by row — what both
 *     orchestrators sort by (PhotoRAGOrchestrator.swift:313, VideoRAGOrchestrator.swift:385-388), and what makes the answer
 *     independent of the store's mutation history and of sharding.
 *  4. The first `limit` groups are returned: out_root_ids[g], and out_root_scores[g] = VectorMetric.score(fromDistance:) of the
 *     group's distance.
 *  5. Within a returned group the per_group best rows by (distance ascending, row ascending), the tie rule of every search route:
 *     out_member_ids[g * per_group + j], out_member_scores likewise. Member 0 is the row that gave the group its distance.
 *  6. Unused member slots are padded with UINT64_MAX / 0.0f; out_member_counts[g] (may be NULL) = members written for group g.
 *  7. With has_min_score, groups whose score is below min_score are dropped, as are members below it (on the host, as elsewhere).
 * out_root_ids / out_root_scores: [limit]. out_member_ids / out_member_scores: [limit][per_group], both NULL = no members wanted.
 * *out_count = groups written. limit <= 0: count 0, no device touched. per_group < 1 is read as 1. An empty engine gives count 0.
 * Refused with the outputs untouched: limit > WAX_HIP_GROUP_MAX_LIMIT, per_group > WAX_HIP_GROUP_MAX_MEMBERS, a NULL engine, query,
 * out_count or root array, one member array without the other, a dimension mismatch (the reference's message). On a store where no
 * parent was ever set the same machinery runs with one group per row; there is no shortcut through wax_hip_search, whose tie rule is
 * by row. All three metrics and every dimension are served: the dimensions of the lane-shape table by one fused pass that offers every
 * row's key to its group's slot by a 64-bit atomic minimum, the others (and "force_general") by the distance column and the same
 * offers. A sharded handle serves per_group == 1: every shard answers `limit` groups, the host keeps the smaller distance per root,
 * sorts by (distance, root id) and takes `limit` — exact, because a root among the global first `limit` is, on the shard that holds
 * its best row, beaten only by roots that beat it globally. per_group > 1 on a handle is refused: a shard that did not rank a root
 * cannot say what its members there are. No allow-list, no ticket form, no batched form. */
int wax_hip_search_grouped(wax_hip_engine* e, const float* query, uint32_t dims, int32_t limit, int32_t per_group,
                           int has_min_score, float min_score, const wax_hip_row_predicate* pred,
                           uint64_t* out_root_ids, float* out_root_scores,
                           uint64_t* out_member_ids, float* out_member_scores,
                           uint32_t* out_member_counts, uint32_t* out_count);
/* What the grouped searches of this engine did, in the way of wax_hip_predicate_ticket_stats (a read-out, no tuning key): searches
 * that reached the device, of which fused_scans took the one-pass scan and column_scans the distance column; member_rounds launched;
 * group_slots of the latest search (rows, on a store without parents); parent_rows_uploaded = rows of the slot column sent to the
 * device so far. A sharded handle reports the sums over its shards (group_slots: the sum of the shards' latest). */
typedef struct wax_hip_group_stats_t {
    uint64_t searches, fused_scans, column_scans, member_rounds, group_slots, parent_rows_uploaded;
} wax_hip_group_stats_t;
int wax_hip_group_stats(wax_hip_engine* e, wax_hip_group_stats_t* out);

/* ---- required-term search: MetadataFilter as a pre-filter ------------------------- */

/* FrameFilter.metadataFilter (SearchRequest.swift:130-145; matches(metadataFilter:meta:), UnifiedSearch.swift:1215-1239) is the sixth
 * test of passesFrameFilter (UnifiedSearch.swift:1241-1258): a conjunction — every requiredEntries[key] == value, every requiredTags
 * pair and every requiredLabels string must be on the frame. The reference applies it to an over-fetched prefix (candidateLimit rows),
 * so a session that owns a small share of a large store (WaxMCPTools.swift:582 scopes every recall by "session_id") gets too few hits
 * or none. Here it is a pre-filter on the device.
 *
 * A TERM is an opaque uint32 the caller chooses: strings do not cross this ABI. The caller owns the dictionary that maps
 * ("entry", key, value), ("tag", key, value) and ("label", s) to ids, so the filter is exact — no hash, no collision. A fourth
 * optional per-row column carries a SET of 0 .. WAX_HIP_TERMS_MAX_PER_ROW distinct terms per row, under the lifecycle of the
 * timestamp, flag and parent columns word for word: a store on which terms were never set allocates nothing and every row holds the
 * empty set; an appended row gets the empty set; an upsert keeps its row's set; removals take the row's set with them; reserve and
 * growth keep the column; a move between shards carries it; wax_hip_deserialize drops it (wax_hip_serialize is unchanged). The host
 * copy is authoritative; the device copy (CSR: uint32 offsets of rows + 1 entries, uint32 values ascending within a row) is brought
 * up to date by the first term search after a change, from the lowest changed row. A store holds fewer than 2^32 terms in all. */
#define WAX_HIP_TERMS_MAX_PER_ROW  64
#define WAX_HIP_TERMS_MAX_REQUIRED 16
/* Replaces the WHOLE set of frame_ids[i] with terms[term_begin[i] .. term_begin[i] + term_len[i]) (the allow_begin / allow_len
 * convention of wax_hip_search_batch_filtered); a length of 0 clears the set; duplicates inside one set collapse. Ids the engine does
 * not hold are skipped, an id listed twice takes its last entry, *out_applied (may be NULL) = entries that named a held frame — as
 * wax_hip_set_attributes. A writer: a thread that holds uncollected search tickets is refused. Refused with NOTHING applied: a set of
 * more than WAX_HIP_TERMS_MAX_PER_ROW terms after de-duplication, a span that leaves [0, n_terms), NULL arrays (terms may be NULL
 * when every length is 0), and (WAX_HIP_ERR_CAPACITY) a call after which the store would hold 2^32 terms or more. The spans and
 * set sizes are checked before the engine is looked at; a sharded handle checks every shard's total before it changes any shard. */
int wax_hip_set_terms(wax_hip_engine* e, const uint64_t* frame_ids, const uint64_t* term_begin, const uint32_t* term_len,
                      const uint32_t* terms, uint64_t n_terms, uint64_t n, uint64_t* out_applied);
/* The set of one frame, ascending: *out_count = its size (also when out_capacity is smaller; then only out_capacity terms are
 * written), *out_found (may be NULL) = 1 for a frame the engine holds, else 0 and count 0. */
int wax_hip_get_terms(wax_hip_engine* e, uint64_t frame_id, uint32_t* out_terms, uint32_t out_capacity, uint32_t* out_count, uint8_t* out_found);
/* wax_hip_search_predicate restricted to the rows whose set contains EVERY one of required_terms[0 .. n_required) (duplicates among
 * them collapse; more than WAX_HIP_TERMS_MAX_REQUIRED distinct ones are refused). The answer is bit for bit what
 * wax_hip_search_predicate returns when its allow-list is the frame ids of exactly those rows, intersected with the caller's list if
 * one is given: ids, scores, count, ties in ascending row order, the score cut on the host. With n_required == 0 the call IS
 * wax_hip_search_predicate (one body, the same launches, the same counters). On a store where no terms were ever set, n_required > 0
 * gives count 0 with no device work (`guard let entries = meta.metadata?.entries else { return false }`, UnifiedSearch.swift:1219).
 * Otherwise term_mask_kernel turns the CSR column into the row bitmap every filter route works from — ANDed into the allow-list
 * probe's where there is a long list — attr_mask_kernel applies the predicate (or passes everything) and counts, and the routes of
 * wax_hip_search_predicate answer: the gather, the masked f32 scan, the masked bf16-mirror scan under its certificate. A list below
 * "filter_device_min" is staged on the host, where the term test reads the host column. The counters and tuning keys are those of
 * the predicate search — of one under a predicate that passes every row where the caller gave none, so a term search charges
 * "predicate_searches" and its route's counter ("predicate_gather_searches", ...) although no attribute was tested;
 * wax_hip_term_stats reads out the rest. Refusals: those of wax_hip_search_predicate in its order, then a NULL
 * required_terms with n_required > 0, then too many distinct terms. Blocking; a reader. A sharded handle runs every shard on its
 * workers and merges as it does for wax_hip_search_predicate. */
int wax_hip_search_terms(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k,
                         int has_allow, const uint64_t* allow_frame_ids, uint64_t n_allow,
                         int has_min_score, float min_score, const wax_hip_row_predicate* pred,
                         const uint32_t* required_terms, uint32_t n_required,
                         uint64_t* out_ids, float* out_scores, uint32_t out_capacity, uint32_t* out_count);
/* What the term searches (n_required > 0) of this engine did, a read-out in the way of wax_hip_group_stats (no tuning key): searches;
 * device_masks = term_mask_kernel launches; host_staged = short lists tested on the host column; host_decided = answered empty
 * because the store never had terms; term_rows_uploaded / term_values_uploaded = offsets' rows and values sent to the device so far.
 * A sharded handle reports the sums over its shards. */
typedef struct wax_hip_term_stats_t {
    uint64_t searches, device_masks, host_staged, host_decided, term_rows_uploaded, term_values_uploaded;
} wax_hip_term_stats_t;
int wax_hip_term_stats(wax_hip_engine* e, wax_hip_term_stats_t* out);
/* wax_hip_search_batch_predicate with a required-term set PER QUERY: query q requires
 * required_terms[term_begin[q] .. term_begin[q] + term_len[q]) (the allow_begin / allow_len convention; length 0 = no term filter for
 * q). Both arrays NULL: no query has one, and the call IS wax_hip_search_batch_predicate — one body, the same launches, the same
 * counters. Row q equals, bit for bit (ids, scores, count, ties in ascending row order),
 * wax_hip_search_terms(e, query q, ..., list q, cut q, &preds[q], terms q, ...) with out_capacity = out_stride.
 * Refusals: those of wax_hip_search_batch_predicate in its order; then one of term_begin / term_len given without the other; then a
 * span that leaves [0, n_required_terms) (or a non-empty span with required_terms NULL); then a set of more than
 * WAX_HIP_TERMS_MAX_REQUIRED distinct terms (duplicates collapse first). The outputs are untouched and the message names the query.
 * Queries whose sets are equal AS SETS — whatever the order or the duplicates — share a set, and with the same list and predicate
 * an entry of the pass. On a store that never had terms every query with a non-empty set gets count 0 without device work.
 * Entries without an allow-list: term_mask_multi_kernel reads the CSR term column ONCE for up to 32 distinct sets (further launches
 * beyond 32) and writes one row bitmap and one passing count per set; the counts are downloaded (one small copy, one synchronisation,
 * only in calls that have such entries), an entry's upper bound is its set's count — not the store's — and a count of 0 ends it; the
 * entries' row lists then come from the three launches of wax_hip_search_batch_predicate with the bitmap ANDed in. Sets are admitted in
 * order of their first query while there are at most 256 of them and their bitmaps fit 256 MiB. Entries with a list of at most 16 384
 * ids: the LDS sort drops a probed row that lacks a required term, beside the predicate test. Queries with a longer list and terms,
 * and those of sets or entries that are not admitted, take wax_hip_search_terms' body under the lock held. A term query is charged as
 * a predicate query is — one without a predicate as one whose predicate passes every row; "predicate_batch_rows" applies to the
 * upper bounds above. A sharded handle runs every shard on its workers and merges as wax_hip_search_batch_predicate does. */
int wax_hip_search_batch_terms(wax_hip_engine* e, const float* queries, uint32_t nq, uint32_t dims, int32_t top_k,
                               const uint64_t* allow_frame_ids, uint64_t n_allow_ids,
                               const uint64_t* allow_begin, const uint64_t* allow_len,
                               const float* min_scores, const wax_hip_row_predicate* preds,
                               const uint32_t* required_terms, uint64_t n_required_terms,
                               const uint64_t* term_begin, const uint32_t* term_len,
                               uint64_t* out_ids, float* out_scores, uint32_t out_stride, uint32_t* out_counts);
/* What the wax_hip_search_batch_terms calls with at least one term query did (no tuning key): calls; queries = term queries answered by
 * the shared pass; sets = distinct term sets sent to the device by those passes; mask_launches = term_mask_multi_kernel launches;
 * looped = term queries answered by the single-query body; host_decided = term queries answered empty because the store never had
 * terms. A sharded handle reports the sums over its shards. */
typedef struct wax_hip_term_batch_stats_t {
    uint64_t calls, queries, sets, mask_launches, looped, host_decided;
} wax_hip_term_batch_stats_t;
int wax_hip_term_batch_stats(wax_hip_engine* e, wax_hip_term_batch_stats_t* out);

/* ---- persistence: "MV2V" vec segment, encoding 2 ------------------------- */

/* serialize() (MetalVectorEngine.swift:682-714): byte-identical layout
 * "MV2V" u16 ver=1 u8 enc=2 u8 similarity u32 dim u64 count u64 vectorBytes 8x0
 * | count*dim f32 LE | u64 idBytes | count u64 LE. */
int wax_hip_serialize(wax_hip_engine* e, uint8_t** out_bytes, size_t* out_len);
/* deserialize(_:) (MetalVectorEngine.swift:716-815), same validation order and reasons. */
int wax_hip_deserialize(wax_hip_engine* e, const uint8_t* bytes, size_t len);
void wax_hip_free(void* p);

/* ---- observability / tuning --------------------------------------------- */

int wax_hip_stats(wax_hip_engine* e, wax_hip_stats_t* out);
/* Tunables (all optional). No key can change an answer: every setting selects between paths that return the same hits.
 *
 * single-query scan
 *   "grid_blocks" (0 = auto), "variant" (scan kernel variant index, -1 = auto), "stream_nt", "force_general" (1 = the distance-buffer +
 *   radix-select path even for small k), "slots" (scratch-slot pool size), "streams" (1..4 in-order streams the slots rotate over),
 *   "time_kernels" (wax_hip_stats' kernel times: 1 = HIP events recorded in front of and behind the scan / filtering-GEMM launch on its own
 *   stream — the interval holds the kernel and the packets around it; 2 = the event pair bound to the dispatch itself (hipExtLaunchKernel):
 *   no trailing marker and no chain wait inside the interval; 4-8 us above rocprofv3's duration of the same dispatch), "reset_stats" (any value: zero the counters),
 *   "fuse_merge" (1 (default) = on grids of at most 160 workgroups the scan kernel's last-arriving workgroup does the final merge),
 *   "merge_kway" (1 (default) = top_k <= 64: that workgroup merges the per-workgroup lists by their heads, which lets every default
 *   grid of a store of up to 2 GiB of rows finish in ONE launch; 0 = the round-3 rule),
 *   "merge_overlap_mb" (default 400: a scan submitted while other single-query tickets of the engine are out — a stream of scans — over a
 *   store of at least this many MB leaves the merge to a second launch, which overlaps the next scan; 0 = never; a query submitted alone
 *   always keeps the single launch), "overlap_scans" (read-only: scans that took that form),
 *   "query_args" (dims 384 / 768: 1 (default) = a scan that merges in its own kernel takes the query in its kernel arguments; 2 = every
 *   store; 0 = never), "scan_plain_mb" (such scans read stores of at most this many MB with ordinary instead of non-temporal loads, default 32),
 *   "done_flag" (1 (default) = such a scan publishes a completion word in coherent pinned memory behind its hits and collect polls it
 *   instead of an event; never while "time_kernels" != 0),
 *   "scan_chain" (pipelined scans of different streams: 1 = chained through an event so that a per-launch duration is one scan alone;
 *   0 = free to overlap; -1 (default) = chained exactly while "time_kernels" != 0), "share_timing" (1 = a chained scan reuses its
 *   predecessor's end event as its start event),
 *   "select_short" (1 (default): top_k > 192 = the fused scan leaves every workgroup's 192 best, ONE workgroup selects the top_k among
 *   them in LDS and certifies that no workgroup dropped one of the answer — otherwise, on the device, the distance pass + radix
 *   selection behind it answers; 64 < top_k <= 192 on grids that do not merge in the scan kernel = the same workgroup is the final
 *   merge (nothing can have been dropped: no certificate), the wave-list merge stays behind it, gated; 0 = the long path / the wave-list
 *   merge at once; 2 = like 1 with 192-entry lists whatever top_k (1 keeps 64-entry lists while top_k <= 8 per workgroup); "force_general"
 *   implies 0 for top_k > 192), "select_grid" (0 (default) = the radix selection's histogram and compaction passes run
 *   min(2048, ceil(rows / 256)) workgroups; 1..2048 = at most that many, so that a thread takes several trips of its loops on a small
 *   store: for tests), "short_selects" / "short_select_failures" (read-only: short selections
 *   enqueued / that left the answer to the launches behind them),
 *   "scan_mirror" (single queries, dims 384 / 768, cosine / dot, top_k <= 32, default variant, no "force_general": 1 (default) = stores of
 *   more than 2 GiB of f32 rows stream the bf16 mirror instead (half the bytes), re-score the 64 best rows in f32 with the f32 scan's
 *   arithmetic and release the answer only under the mirror's certificate — otherwise collect re-runs the query on the f32 scan; 2 = every
 *   such store; 0 = never), "mirror_scans" / "mirror_scan_fallbacks" / "mirror_scan_unavailable" (read-only: single queries that took the
 *   mirror / whose certificate failed and were re-run on the f32 scan / that took the f32 scan because the mirror could not be prepared),
 *   "mirror_share" (single queries in flight share passes over the mirror, up to 4 per pass, each answered exactly as it would be alone:
 *   1 (default) = a query submitted while a mirror pass of this engine is still running is parked — the ticket is returned, nothing is
 *   launched — and launched together with whatever else is parked when four are parked, when a collect is about to block, or by a submit
 *   that finds no pass running; a lone query launches at once; 2 = always parked until a collect needs the answer or four are parked;
 *   0 = never, one pass per query. Nothing is parked while "time_kernels" != 0 or scans are chained), "mirror_passes" /
 *   "mirror_shared_passes" / "mirror_shared_queries" (read-only: scan launches over the mirror / of which with two or more queries /
 *   queries those answered; "mirror_scans" keeps counting queries),
 *   "mirror_fill" (under "mirror_share" 1: 1 (default) = a caller who pipelines single queries gets full passes — a submit is also parked
 *   when this engine has mirror tickets that are launched and not yet collected (a pass in flight, or finished tickets whose caller is
 *   draining a pass and submits again at once), and a set that is not full is launched only by the collect of one of its own tickets or
 *   by a submit that finds no such ticket; a collect that blocks on a running ticket holds it back. A query submitted behind finished
 *   uncollected tickets by a caller who then stays away waits for that caller's next collect. 0 = the eager rule described under
 *   "mirror_share"), "mirror_fill_holds" (read-only, counted under "mirror_fill" 1 only. A submit counts when no pass was in flight and
 *   the eager rule would have launched there — the query alone, or the parked set it joined — and the rule left it parked behind a
 *   launched uncollected ticket instead; a submit parked behind a pass in flight is parked under either rule and does not count, nor
 *   does the submit that fills a set. A collect counts when it was about to block on a running ticket of another pass while a set was
 *   parked and left that set parked),
 *   "mirror_bits" (which mirror a single query that takes one streams: 0 (default) = auto — where "scan_mirror" is 1, the store holds more
 *   than 2 GiB of f32 rows and top_k <= 16, the 8-bit code mirror: one byte per element, row-scaled, plus {scale, err} per row, built from
 *   the f32 store (rows x (dims + 8) bytes). A row's key is a lower bound of its distance from its own measured error, the 64 best are
 *   re-scored in f32 and the answer is released only under the certificate, else collect re-runs the query on the f32 scan as for bf16;
 *   everything else takes the bf16 mirror. 8 = the code mirror wherever a mirror is taken and top_k <= 16; 16 = always bf16. Appended rows
 *   are converted at the next query; any other mutation makes the code mirror stale as a whole, and a stale or missing one is rebuilt by
 *   the third eligible query in a row since the last mutation — the first two take bf16. A parked set rides one mirror: bf16 if any member
 *   has top_k > 16. Breaker: when 8 of the engine's last 32 8-bit queries were uncertified the next 1024 eligible queries take bf16),
 *   "mirror8_passes" / "mirror8_fallbacks" / "mirror8_unavailable" / "mirror8_conversions" / "mirror8_rows_converted" /
 *   "mirror8_breaker_trips" (read-only: scan launches over the code mirror, also counted in "mirror_passes" / 8-bit queries re-run on the
 *   f32 scan, also in "mirror_scan_fallbacks" / queries sent to bf16 because the code mirror could not be allocated or converted /
 *   conversions enqueued / rows they converted / times the breaker opened),
 *   "filter_device_min" (wax_hip_search_filtered: allow-lists at least this long are resolved by the id -> row table in HBM, default 4096; -1 = never),
 *   "filter_batch" (wax_hip_search_batch_filtered: 1 (default) = one gather pass for all allow-lists; 0 = the single-query filtered path
 *   per query), "filter_batch_queries" / "filter_batch_fallbacks" (read-only: listed queries answered by the gather pass / by the
 *   per-query path; wax_hip_search_batch_predicate counts its queries with a predicate and no list here too),
 *   "predicate_batch_rows" (wax_hip_search_batch_predicate: row slots one call may spend on entries with a predicate, 0..2^31-1;
 *   default 67108864 = 256 MB of row indices, a memory cap and not a tuned number; entries beyond it take the single-query predicate
 *   search), "predicate_batch_queries" / "predicate_batch_classes" (read-only: queries with an effective predicate — not empty, and not
 *   decided on the host for a store without attributes — that the batched gather pass answered / entries with a predicate it built;
 *   "predicate_searches" counts such queries whatever the route),
 *   "search_many" (wax_hip_search_many: 1 (default) = this engine's pairs may share the call's pooled launch; 0 = each runs the
 *   single-query search), "search_many_max_rows" (engines holding more rows than this always take the single-query search; default
 *   262144, the first power of two above the vec segment cap at 384-d), "search_many_pooled" / "search_many_looped" (read-only: pairs
 *   of this engine answered by the pooled launch / by the single-query search), "search_many_masked" (read-only: pairs of
 *   wax_hip_search_many_predicate answered by a pooled group that read a row bitmap — a non-empty predicate evaluated on the device).
 * batched queries (bf16 MFMA GEMM + fused selection + exact re-score; exact answers whatever the setting)
 *   "batch_mode" (0 = never use the MFMA path), "batch_min" (smallest batch that may use it, default 1; below 16 queries a cost model
 *   picks between one GEMM pass over the bf16 mirror and nq f32 scans), "batch_workspaces" (concurrent batched searches per engine, default 4),
 *   "batch_qfrag" (1 (default) = the register-resident GEMM loads its query fragments from a fragment-ordered copy the prep kernel writes —
 *   coalesced 1-KB runs; 0 = from the row-major block),
 *   "batch_rega" (1 (default) = the register-resident-queries GEMM with a workgroup barrier per tile; 5 = the same with the split
 *   tile barrier (round 5's default); 0 = the LDS-tiled GEMM only), "batch_dyn_tail" (1 (default) = with up to 256 queries per pass the workgroups of the
 *   filtering GEMM claim the last twelfth of the store's tiles from a pool, so the launch ends within one tile of every workgroup; 0 = fixed shares), "batch_onepass" (0 = always the slab pipeline), "batch_onepass_tiles" (smallest store, in
 *   units of 64 rows — 32 at D = 768 —, that the one-pass pipeline takes; default 64 = 4 096 rows (1024 before round 6), at least 32), "batch_survivors" (floor of the expected survivors per query as a
 *   multiple of k', default 3), "batch_sample_div" (1 / this of the tiles are sampled for the thresholds, default 32),
 *   "batch_retry" (an uncertified query gets ALL of its survivors re-scored before the exact path: 1 (default) = by a device-side
 *   kernel while "retry_hint" > 0 — armed for 16 batches by any such query, settable 0..1024 — and from the host for what is left;
 *   2 = from the host only; 0 = never), "batch_kp_fused" (1 (default) = top_k 81 .. 128 re-scores k' = 192 candidates in the fused finish kernel),
 *   "batch_multi" (1 (default) = uncertified queries share passes over the f32 store, up to 16 per pass, bit-identical to the
 *   single-query kernel), "batch_eps_measured" (1 (default) = the certificate bound uses the measured bf16 rounding errors; 0 = the
 *   worst case 2^-7 per product), "batch_slab_mb" / "batch_growth" / "batch_first" (slab schedule of the slab pipeline),
 *   "batch_debug" (test / diagnosis bits: 4096 = no pace gate in the 768-d filtering GEMM, 16384 = one wave of workgroup 1 pretends its
 *   split-barrier wait timed out (its workgroup's queries take the exact path), 65536 = the device-side retry re-scores every
 *   survivor; any other bit is refused), "batch_prof_ptr" (diagnosis: device address of a [256 x 8][20] u32 buffer — the filtering GEMM at
 *   D = 384 / 768 then runs its phase-timing build, which leaves per-wave s_memtime cycle counts there, same answers, ~10 % slower;
 *   0 (default) = the product kernel; tools/gemm_phase_budget.py),
 *   "batch_host_multi" (host-pointer batches of at least 16 queries that the MFMA pipelines do not take — top_k 81 .. 192 on a store below
 *   the one-pass floor, "batch_mode" 0 —: 1 (default) = up to 16 queries share one exact pass over the f32 store, bit-identical to the
 *   single-query kernel; 0 = one scan per query),
 *   "batch_in_wait" (device-resident batches: 0 (default) = the library's stream is ordered behind the caller's `stream` by an event
 *   only while that stream still has work pending — a drained stream costs no marker / barrier packet; 1 = always, as before round 6).
 * removeBatch (wax_hip_remove_batch)
 *   "compact_window_rows" (source rows per window of the compaction pass; 0 (default) = as many as the bounce buffer holds of every
 *   per-row array at once, larger values are capped there; a window whose shift is below its length goes through the bounce buffer,
 *   one whose shift has reached this many rows moves directly and is as long as its shift),
 *   get-only "remove_batches" (calls that removed rows in one pass), "remove_batch_rows" (rows they removed),
 *   "remove_batch_bytes_written" (device bytes their passes wrote, bounce writes included).
 * predicate search (wax_hip_search_predicate)
 *   "predicate_route" (0 (default) = auto, 1 = always gather the passing rows — bitmap -> compact row list -> exact distances of the
 *   listed rows -> general selection —, 2 = the masked f32 scan wherever it is eligible: top_k <= 192, a specialised dimension, no
 *   "force_general"), "predicate_scan_min_permille" (the auto rule: the masked scan when at least this many rows per thousand pass;
 *   default 500: where the first build's routes crossed for a random mask, between 1/8 and 1/2 passing; at 10M rows the committed
 *   f32 scan crosses the gather between 1/2 and 15/16, the mirror form between 1/8 and 1/2: DESIGN 4.5),
 *   "predicate_mirror" (a form of the masked scan, not a route of its own: where "predicate_route" sends a query to the masked scan,
 *   cosine or dot at 384 / 768 dimensions, top_k <= 32, the default "variant", "grid_blocks" <= 512 and more than 64 rows pass, the scan
 *   streams the bf16 mirror under the bitmap — 16 / 8 rows per chunk —, the 64 best approximate keys among the passing rows are re-scored
 *   in f32, and the answer is returned only under the single-query mirror scan's certificate: then it is the masked f32 scan's bit for
 *   bit; otherwise the masked f32 scan answers on the same bitmap. 0 = never; 1 (default) = auto: stores of more than 2 GiB of f32 rows
 *   while "scan_mirror" != 0; 2 = every store; other values are refused. A mirror that cannot be allocated or converted sends the query
 *   to the f32 scan: no query fails because of it),
 *   get-only "predicate_mirror_scans" / "predicate_mirror_fallbacks" / "predicate_mirror_unavailable" (masked scans answered from the
 *   mirror under the certificate / re-run on the masked f32 scan because the certificate failed / sent there because the mirror could
 *   not be prepared; each of them counts once in "predicate_masked_scans"),
 *   get-only "predicate_searches" (calls with a non-empty predicate), "predicate_gather_searches" / "predicate_masked_scans" (those
 *   answered by either route; a call whose predicate no row passes counts in neither), "predicate_chunks_skipped" (chunks of rows the
 *   masked scans did not load), "attr_uploaded_rows" (rows of the attribute columns uploaded so far — an append uploads its own rows
 *   only), "attr_device_rows" (rows the device columns are allocated for; 0 = the store never had attributes). wax_hip_stats'
 *   bytes_scanned counts what a predicate search actually read: the gathered rows, or every row of the chunks it did not skip (the
 *   mirror form: its chunks at two bytes per element plus the 64 re-scored f32 rows, and the f32 scan's figures on top when the
 *   certificate failed; "predicate_chunks_skipped" then counts the mirror's chunks, and the f32 scan's too on a fallback).
 * get-only
 *   "variant_count", "scan_grid", "store_ptr" (device address of the f32 slab), "fused_max_k", "batch_queries", "query_args_scans", "merged_scans", "done_flag_waits",
 *   "batch_inline_retries", "batch_max_row_err_e9", "batch_fallbacks", "onepass_queries", "batch_max_k", "batch_retries",
 *   "batch_multi_passes", "batch_multi_queries", "batch_multi_group" / "batch_multi_group_big", "filter_device_searches",
 *   "mirror_rows_converted" / "mirror_conversions" (bf16 mirror: rows converted / conversions enqueued so far — an append converts its own
 *   rows only), "idhash_rows_inserted", "batch_max_norm_e6".
 * sharded handles: every key above is forwarded to all shards; plus
 *   "ticket_path" (single queries: 1 (default) = every shard that holds rows answers through its own ticket — one launch per shard,
 *   submitted side by side by the handle's worker threads, hits straight to pinned memory — and the host merges G x k keys;
 *   0 = the device gather below), "exchange" (device gather: 0 = peer copies + merge on the first device, 1 = one RCCL all-gather per
 *   query; 1 implies the device gather), "gather" (0 = device; 2 = through the host: what a handle falls back to when a device pair
 *   lacks peer access), "shard_min_mb" (a shard's block holds at least this many MB of rows, default 64: a store below it lives on
 *   the first device only; 0 = spread from the first row; env WAX_HIP_SHARD_MIN_MB sets the default),
 *   get-only "shards", "block_rows", "rebalances", "rccl_collectives", "rccl_ranks" (ncclCommCount of the in-library communicator),
 *   "peer_pairs" / "peer_enabled", "ticket_searches" / "single_shard_searches" / "inline_fanouts" (single-query fan-outs submitted from the caller's thread because the workers were busy with a long job), "parallel_submits", "parallel_collects". */
int wax_hip_set_tuning(wax_hip_engine* e, const char* key, int64_t value);
int64_t wax_hip_get_tuning(wax_hip_engine* e, const char* key);
/* Times `iters` back-to-back launches of ONLY the scan kernel for `query`
 * with HIP events on the engine's stream; returns average ms per launch
 * (kernel sweeps; bench.py's roofline uses the per-launch events of its timed
 * region instead: "time_kernels" + wax_hip_stats). */
int wax_hip_time_scan_kernel(wax_hip_engine* e, const float* query, uint32_t dims, int32_t top_k,
                             uint32_t iters, double* out_avg_ms);
/* Pure streaming-read microbenchmark over the engine's own store (sum of all
 * float4s, no top-k): the node's achievable read bandwidth for this layout. */
int wax_hip_time_stream_read(wax_hip_engine* e, uint32_t iters, double* out_avg_ms);
/* Diagnostic read-out of the 8-bit code mirror ("mirror_bits"; tests hold the conversion kernel and its upkeep to a float64
 * reference through it; no product path calls it). Copies what the device holds for rows [first_row, first_row + n_rows):
 * out_codes = n_rows * dims biased bytes (code + 128) as stored, out_meta = n_rows * 2 floats {scale, err}; *out_max_norm = the
 * mirror's max-norm word, *out_rows_coded = the number of rows coded. n_rows == 0 reports the last two only (out_codes and
 * out_meta may then be NULL). It never builds or refreshes the mirror, waits for a conversion still in flight, and changes no
 * counter and no breaker state. WAX_HIP_ERR_INVALID_ARGUMENT: a sharded handle, a code mirror that is absent or not valid (after
 * any mutation, until a query has rebuilt it), a range beyond the coded rows, a needed pointer that is NULL. */
int wax_hip_mirror8_snapshot(wax_hip_engine* e, uint64_t first_row, uint64_t n_rows, uint8_t* out_codes, float* out_meta,
                             float* out_max_norm, uint64_t* out_rows_coded);
/* Diagnostic read-out of the 8-bit pass's keys (tests hold the scan's arithmetic to an integer model through it; no product path
 * calls it): out_keys[r] = the f32 key — a lower bound of the distance, -inf for a row that is always a candidate — that the lone
 * 8-bit scan computes for `query` (dims floats) at coded row r, by the scan's own body. n_keys must equal the number of rows coded
 * (wax_hip_mirror8_snapshot's *out_rows_coded). It never builds or refreshes the mirror, waits for a conversion still in flight,
 * and changes no counter and no breaker state. WAX_HIP_ERR_INVALID_ARGUMENT: a sharded handle, a code mirror that is absent or not
 * valid, another n_keys, a NULL pointer. */
int wax_hip_mirror8_keys(wax_hip_engine* e, const float* query, float* out_keys, uint64_t n_keys);
/* Diagnostic of the mirror finish's candidate selection (tests compare its two ways through it; no product path calls it). `lists`
 * = n_lists (1 to 512) lists of 64 keys each, every list ascending and padded with INT64_MAX, no key twice. On the current device,
 * in one workgroup with the finish's own shared-memory layout: out_selected[64] = the 64 smallest keys as the finish picks them
 * (the gathered prefixes where they fit its buffer, else the k-way merge), out_merged[64] = the k-way merge alone, *out_gathered =
 * 1 where the gather answered. Blocking. */
int wax_hip_mirror_select_probe(const int64_t* lists, uint32_t n_lists, int64_t* out_selected, int64_t* out_merged, int32_t* out_gathered);
/* Diagnostic of the selection frame of a mirror pass — the wave lists, their prunes and the workgroup merge — on keys the caller
 * makes up (tests hold it to a host model through it; no product path calls it). `keys` = nq (1 to 4) arrays of n_slots (1 to 2^24)
 * keys, one per row slot and query; INT64_MAX marks a slot that is not offered to that query (a tail row, a masked row), and no
 * other key occurs twice in one array. On the current device a launch of `grid` (1 to 8) workgroups walks the slots as a pass walks
 * its 16-row tiles: wave g of the 4 * grid takes slots [16 c, 16 c + 16) for c = g, g + 4 * grid, ... and offers each query its
 * keys there. out_partials[(q * grid + b) * 64 ..] = the 64 keys workgroup b keeps for query q: the smallest it was offered,
 * ascending, INT64_MAX behind them. Blocking. */
int wax_hip_mirror_lists_probe(const int64_t* keys, uint32_t nq, uint64_t n_slots, uint32_t grid, int64_t* out_partials);
/* Diagnostic of the timeline's two kernels on columns the caller makes up (tests make one workgroup walk many tiles and cut its buffer
 * several times on a few thousand rows through it; no product path calls it, no tuning key exists for its grid). Host columns of
 * n_rows (< 2^32) rows — timestamps NULL / flags NULL = zeros, frame_ids distinct — are uploaded to the current device, the selection
 * runs with `grid` workgroups (0 = the product's own choice, at most 1 024) and the merge behind it, and out_ids[limit] (padded with
 * UINT64_MAX), out_timestamps[limit] (may be NULL; padding 0) and *out_count come back. limit <= 0 gives count 0 and touches no
 * device; limit > WAX_HIP_TIMELINE_MAX_LIMIT is refused. Blocking. */
int wax_hip_timeline_probe(const int64_t* timestamps, const uint32_t* flags, const uint64_t* frame_ids, uint64_t n_rows,
                           int32_t limit, int newest_first, const wax_hip_row_predicate* pred, uint32_t grid,
                           uint64_t* out_ids, int64_t* out_timestamps, uint32_t* out_count);
/* Diagnostic of the grouped search's selection on distances the caller makes up (tests set them bit for bit; no product path calls it).
 * Host columns of n_rows (< 2^32) rows — distances, slots (NULL = every row its own slot, n_slots >= n_rows), slot_root[n_slots]
 * (NULL = the slot's number), bitmap of ceil(n_rows / 32) words (NULL = every row takes part) — are uploaded to the current device;
 * the column route's offer kernel and the member rounds run with `grid` workgroups (0 = the product's own choice, at most 1 024),
 * the selection and the marking between them. Back come out_root_ids[limit] (padded with UINT64_MAX), out_root_keys[limit] (each
 * group's best key, distance bits : row; padding INT64_MAX), out_member_keys[limit][per_group] (may be NULL; padding INT64_MAX) and
 * *out_count. limit <= 0 gives count 0 and touches no device; limit > WAX_HIP_GROUP_MAX_LIMIT, per_group outside
 * 1 .. WAX_HIP_GROUP_MAX_MEMBERS and a slot >= n_slots are refused. Blocking. */
int wax_hip_group_probe(const float* distances, const uint32_t* slots, const uint64_t* slot_root, const uint32_t* bitmap,
                        uint64_t n_rows, uint32_t n_slots, int32_t limit, int32_t per_group, uint32_t grid,
                        uint64_t* out_root_ids, int64_t* out_root_keys, int64_t* out_member_keys, uint32_t* out_count);
/* Diagnostic of term_mask_kernel on a column the caller makes up (tests drive many grid-stride iterations and every span shape
 * through it without a large store; no product path calls it). offsets[n_rows + 1] (non-decreasing, n_rows < 2^32) and
 * values[offsets[n_rows]] are uploaded to the current device, ONE launch of exactly `grid` workgroups (1 .. 1 024) writes
 * out_bitmap[ceil(n_rows / 32)]: bit r = "row r's values contain all of required[0 .. n_required)" (1 .. WAX_HIP_TERMS_MAX_REQUIRED
 * terms, duplicates collapse), ANDed with bitmap_in where that is not NULL; bits at and beyond n_rows are clear. Blocking. */
int wax_hip_term_mask_probe(const uint32_t* offsets, const uint32_t* values, uint64_t n_rows, const uint32_t* required, uint32_t n_required,
                            const uint32_t* bitmap_in, uint32_t grid, uint32_t* out_bitmap);
/* The same for term_mask_multi_kernel: n_sets (1 .. 32) term sets, set s = required[set_begin[s] .. set_begin[s] + set_len[s]) (1 ..
 * WAX_HIP_TERMS_MAX_REQUIRED distinct terms each, duplicates collapse; a row's values must be distinct), ONE launch of exactly `grid`
 * workgroups (1 .. 1 024) writes out_bitmaps[n_sets][ceil(n_rows / 32)] and out_counts[n_sets] = the rows that pass each set. Blocking. */
int wax_hip_term_mask_multi_probe(const uint32_t* offsets, const uint32_t* values, uint64_t n_rows, const uint32_t* required,
                                  const uint64_t* set_begin, const uint32_t* set_len, uint32_t n_sets, uint32_t grid,
                                  uint32_t* out_bitmaps, uint32_t* out_counts);

#ifdef __cplusplus
}
#endif
#endif /* WAX_HIP_H */
