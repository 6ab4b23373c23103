// shard_merge.h — how the answers of G shards become the handle's one answer. The shards hold contiguous blocks of the global
// row order, and each has answered with ITS best `limit`; every merge below then gives exactly what one engine holding all the rows gives.
// Plain C++17 over the standard library: no HIP and no project header (the hit type and the pad key are parameters).
// tests/shard_merge/driver.cpp holds each merge to a model over all rows, split into blocks of random sizes, empty ones included.
//
//   merge                       order                                                        what a shard hands in
//   key_merge_add / _cut        ascending key (keys carry the global row: unique, total)     a run of hits, pads anywhere in it skipped
//   merge_by_score              descending score, stable: shard then position on ties        ids and scores, best first
//   merge_timeline              (timestamp, frame id), signed then unsigned; newest first    ids and timestamps, `stride` apart per shard
//                               reverses the timestamp (~t) and not the id
//   GroupMerge                  (distance bits, root id), signed then unsigned; per root     offer(root, best) in shard order
//                               the smaller bits, the lower shard on equal bits
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

// ---- by key: add every shard's run, then cut ----
template <typename Hit, typename Key>
void key_merge_add(std::vector<Hit>& all, const Hit* run, size_t n, Key pad) {
    for (size_t i = 0; i < n; ++i)
        if (run[i].key != pad) all.push_back(run[i]);
}
template <typename Hit>
void key_merge_cut(std::vector<Hit>& all, size_t limit) {
    std::sort(all.begin(), all.end(), [](const Hit& a, const Hit& b) { return a.key < b.key; });
    if (all.size() > limit) all.resize(limit);
}

// ---- by score: the shards' answers to one query, in shard order ----
struct ShardAnswer { const uint64_t* ids; const float* scores; uint32_t n; };
struct ShardHit { float score; uint64_t id; };
// Returns the results written: at most `limit` and at most `capacity`. `all`: scratch, reused by a caller that merges many queries.
inline uint32_t merge_by_score(const std::vector<ShardAnswer>& parts, uint32_t limit, uint32_t capacity, uint64_t* out_ids, float* out_scores,
                               std::vector<ShardHit>& all) {
    all.clear();
    for (const ShardAnswer& p : parts)
        for (uint32_t i = 0; i < p.n; ++i) all.push_back(ShardHit{p.scores[i], p.ids[i]});
    std::stable_sort(all.begin(), all.end(), [](const ShardHit& a, const ShardHit& b) { return a.score > b.score; });
    uint32_t m = 0;
    for (; m < all.size() && m < limit && m < capacity; ++m) { out_ids[m] = all[m].id; out_scores[m] = all[m].score; }
    return m;
}

// ---- timeline: shard g's counts[g] pairs start at ids[g * stride], ts[g * stride]; out_ts may be null ----
inline uint32_t merge_timeline(const uint64_t* ids, const int64_t* ts, const uint32_t* counts, size_t G, size_t stride, bool newest_first,
                               size_t limit, size_t capacity, uint64_t* out_ids, int64_t* out_ts) {
    std::vector<std::pair<int64_t, uint64_t>> all;
    for (size_t g = 0; g < G; ++g)
        for (uint32_t i = 0; i < counts[g]; ++i) all.emplace_back(newest_first ? ~ts[g * stride + i] : ts[g * stride + i], ids[g * stride + i]);
    std::sort(all.begin(), all.end());                       // lexicographic: signed t', then unsigned frame id
    const size_t n = std::min(all.size(), std::min(limit, capacity));
    for (size_t i = 0; i < n; ++i) {
        out_ids[i] = all[i].second;
        if (out_ts) out_ts[i] = newest_first ? ~all[i].first : all[i].first;
    }
    return (uint32_t)n;
}

// ---- grouped: the best member per root over all shards, then the first `limit` roots ----
struct GroupBest { int64_t dist; int64_t key; uint64_t member; };   // ordered distance bits; the member's key and frame id
class GroupMerge {
  public:
    void offer(uint64_t root, const GroupBest& b) {          // in shard order: an equal distance keeps the earlier (lower) shard's
        auto it = by_root_.find(root);
        if (it == by_root_.end()) by_root_.emplace(root, b);
        else if (b.dist < it->second.dist) it->second = b;
    }
    std::vector<std::pair<int64_t, uint64_t>> first(size_t limit) const {   // (distance bits, root)
        std::vector<std::pair<int64_t, uint64_t>> order;
        order.reserve(by_root_.size());
        for (const auto& kv : by_root_) order.emplace_back(kv.second.dist, kv.first);
        std::sort(order.begin(), order.end());               // lexicographic: signed distance bits, then unsigned root id
        if (order.size() > limit) order.resize(limit);
        return order;
    }
    const GroupBest& best(uint64_t root) const { return by_root_.find(root)->second; }

  private:
    std::map<uint64_t, GroupBest> by_root_;
};
