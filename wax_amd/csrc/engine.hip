// engine.hip — host side of libwaxhip: the HBM-resident store, the scratch-slot pool,
// the reader/writer lock and the C ABI declared in include/wax_hip.h.
//
// Behaviour follows MetalVectorEngine (Sources/WaxVectorSearch/MetalVectorEngine.swift),
// re-designed for a discrete MI355X: the store is one hipMalloc slab [capacity x dims] f32
// row-major (+ a u64 frame-id table beside it so id mapping also happens on device), queries
// travel through pinned staging, every search runs on a pooled scratch slot with its own HIP
// stream (the analogue of the transient buffer pool, :84-117), and there is no CPU fallback.
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "kernels.h"
#include "mirror8_layout.h"
#include "row_columns.h"
#include "derived_rows.h"
#include "work_pool.h"
#include "rw_lock.h"
#include "shard_workers.h"
#include "id_map.h"
#include "shard_layout.h"
#include "shard_merge.h"

using namespace wax;


// ---------------------------------------------------------------------------------------------------------------------------
// ONE translation unit, cut into the files below (round 6: the 3 300-line engine.hip hid the contract). Each .inc is a stretch of
// this file as it stood — included here, in this order, and never compiled on its own: the order is the declaration order, the
// anonymous namespace and the extern "C" block open and close where they always did. row_columns.h, included above, is the one part
// that stands alone: the per-row columns on the host, plain C++ without HIP, tested on the CPU (tests/row_columns/driver.cpp).
// derived_rows.h stands alone in the same way: how far the bf16 mirror, the code mirror and the id table have followed the store
// (tests/derived_rows/driver.cpp). So does the host-side concurrency, which may use threads and mutexes but no HIP: work_pool.h (the pools
// of per-call workspaces and the ticket tables), rw_lock.h (the reader/writer lock, the tickets per submitting thread), shard_workers.h
// (the hand-off to the per-shard threads) and id_map.h (frame id -> row), each with a driver under tests/<name>/driver.cpp. And so do the
// host rules of the sharded handle, which need neither a device nor an engine: shard_layout.h (the block size, the tail shard, the moves of
// a doubling, what a reserve asks of each shard, the slices of a loaded segment, the bases — all from the shards' row counts) and
// shard_merge.h (G shards' answers -> one: by key, by score, timeline pairs, grouped roots), with drivers of their own.
//
//   engine_types.inc       types of the host side: error state, the device guard, scratch slots, workspaces, the device side of the mirrors and the id table, `struct wax_hip_engine`, ticket ownership
//   store_internal.inc     the store behind the C ABI: clampTopK, the scratch-slot pool, the general-selection workspace, staged appends, growth (MetalVectorEngine.swift:84-117, 330-357, 842-890)
//   search_internal.inc    one query -> one scan: which launch form a scan takes and how it is enqueued (`enqueue_scan`), hits -> results (MetalVectorEngine.swift:446-627, VectorMetric.swift:32-43)
//   batch_host.inc         batched queries, host side: the incremental bf16 mirror and id table, pooled batch workspaces, the one-pass planner, the launch chain (`batch_enqueue`) and the exactness ladder behind it
//   api_store.inc          C ABI: availability, create / destroy, accessors, reserve / add / add_batch / add_batch_device / apply_put_embeddings / remove / remove_batch
//   api_search.inc         C ABI: search_submit / search_collect / search, result capacity; the routing of predicate tickets
//   api_batch.inc          C ABI: search_batch[_hits], the device-resident and ticketed batched entry points
//   api_shard.inc          C ABI: the one-rank-per-GPU entry points (set_row_base, search_shard_device, merge_hits_device, merge_batch_hits_device, hits_to_results)
//   api_fusion_filter.inc  C ABI: reciprocal-rank fusion
//   api_predicate.inc      C ABI: per-row attributes (set / get) and their device columns
//   api_terms.inc          C ABI: wax_hip_set_terms / get_terms, wax_hip_search_terms, wax_hip_term_stats, wax_hip_term_mask_probe — the CSR term column and its device copy; the search itself is filter_host.inc's locked body with the term mask in front (UnifiedSearch.swift:1215-1239)
//   filter_host.inc        C ABI: the filtered searches — one query with an allow-list and / or a row predicate (one locked body), the batched allow-list form
//   search_many.inc        C ABI: wax_hip_search_many[_predicate] — one query each against many stores of one device under one snapshot, the eligible pairs in one pooled launch, with a row predicate and a score cut per pair
//   api_timeline.inc       C ABI: wax_hip_timeline[_device | _probe] — the newest / oldest passing rows by (timestamp, frame id), selected on the device from the attribute columns (TimelineQuery.swift:38-53)
//   api_grouped.inc        C ABI: wax_hip_set_parents / get_parents, wax_hip_search_grouped, wax_hip_group_stats, wax_hip_group_probe — the parent column and the best roots by their best member, members per root (PhotoRAGOrchestrator.swift:264-317, VideoRAGOrchestrator.swift:273-417)
//   codec.inc              C ABI: MV2V encoding-2 serialize / deserialize (MetalVectorEngine.swift:682-815)
//   tuning.inc             C ABI: stats, the tuning registry (set / get), the two timing microbenchmarks
//   sharded.inc            the multi-GPU handle (one engine per device behind one handle): streams, peer copies, RCCL, events, workspaces, one fan-out over the shards and one id router; its layout decisions are shard_layout.h's, its host merges shard_merge.h's
// ---------------------------------------------------------------------------------------------------------------------------
#include "engine_types.inc"
#include "store_internal.inc"
#include "search_internal.inc"
#include "batch_host.inc"
#include "api_store.inc"
#include "api_search.inc"
#include "api_batch.inc"
#include "api_shard.inc"
#include "api_fusion_filter.inc"
#include "api_predicate.inc"
#include "api_terms.inc"
#include "filter_host.inc"
#include "search_many.inc"
#include "api_timeline.inc"
#include "api_grouped.inc"
#include "codec.inc"
#include "tuning.inc"
}  // extern "C"

#include "sharded.inc"

