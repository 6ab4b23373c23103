// Stand-alone driver of wax_amd/csrc/shard_merge.h (no HIP, no GPU): the four host merges of a sharded handle against ONE engine. Each case
// draws one engine's rows, splits them into G contiguous blocks of random sizes (empty ones included), lets every block answer with ITS
// best `limit` by the engine's own order, merges the answers and compares with the model's best `limit` over all rows, exactly.
// G = 1 .. 9, seeded. Prints one `state NAME COUNT` line per state and a final `ok:` line; any disagreement prints FAILED and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <limits>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "shard_merge.h"

namespace {

const char* const kStates[] = {
    "key_fewer_rows_than_limit", "key_pads_in_the_middle", "key_pads_inside_a_run", "key_limit_1", "key_empty_shard", "key_more_rows_than_limit",
    "score_ties_across_shards", "score_ties_inside_a_shard", "score_capacity_below_limit", "score_capacity_0", "score_scratch_reused",
    "timeline_newest_first", "timeline_oldest_first", "timeline_equal_timestamps_by_id", "timeline_extreme_timestamps",
    "timeline_ids_from_2_63", "timeline_capacity_below_limit", "timeline_without_timestamps_out",
    "grouped_root_in_several_shards_different_bits", "grouped_root_in_several_shards_equal_bits", "grouped_negative_bits",
    "grouped_more_roots_than_limit", "grouped_with_members", "grouped_without_members",
};
std::map<std::string, unsigned long long> g_entered;
void enter(const std::string& s) { g_entered[s] += 1; }

[[noreturn]] void die(const char* what, int line) {
    std::printf("FAILED: %s (line %d)\n", what, line);
    std::fflush(stdout);
    std::_Exit(1);
}
#define CHECK(c) do { if (!(c)) die(#c, __LINE__); } while (0)

using Rng = std::mt19937_64;
uint64_t upto(Rng& rng, uint64_t n) { return (uint64_t)(rng() % (n + 1)); }

// n rows in G contiguous blocks: the first row of each block and n at the end; some blocks empty
std::vector<size_t> split(Rng& rng, size_t n, size_t G) {
    std::vector<size_t> cut{0};
    for (size_t g = 1; g < G; ++g) cut.push_back(upto(rng, 3) == 0 ? cut.back() : (size_t)upto(rng, n));
    std::sort(cut.begin(), cut.end());
    cut.push_back(n);
    return cut;
}

// ---- by key ----------------------------------------------------------------------------------------------------------------------------
struct Hit { int64_t key; uint64_t id; };
constexpr int64_t kPad = std::numeric_limits<int64_t>::max();

void by_key(Rng& rng, size_t G, size_t n, size_t limit, bool holes) {
    std::vector<Hit> rows;                                   // keys carry the global row: unique
    for (size_t r = 0; r < n; ++r) rows.push_back(Hit{(int64_t)((upto(rng, 40) << 20) | r) - (20ll << 20), 7 * r + 1});
    const std::vector<size_t> cut = split(rng, n, G);
    std::vector<Hit> all;
    bool pads_in_the_middle = false, empty_shard = false;
    for (size_t g = 0; g < G; ++g) {
        std::vector<Hit> mine(rows.begin() + (long)cut[g], rows.begin() + (long)cut[g + 1]);
        std::sort(mine.begin(), mine.end(), [](const Hit& a, const Hit& b) { return a.key < b.key; });
        if (mine.size() > limit) mine.resize(limit);
        empty_shard = empty_shard || mine.empty();
        std::vector<Hit> run;                                // `limit` entries: the hits, pads behind them (or, `holes`, between them)
        for (const Hit& h : mine) {
            if (holes && upto(rng, 2) == 0) run.push_back(Hit{kPad, ~0ull});
            run.push_back(h);
        }
        while (run.size() < limit) run.push_back(Hit{kPad, ~0ull});
        if (mine.size() < limit && cut[g + 1] < n) pads_in_the_middle = true;
        key_merge_add(all, run.data(), run.size(), kPad);
    }
    key_merge_cut(all, limit);
    std::sort(rows.begin(), rows.end(), [](const Hit& a, const Hit& b) { return a.key < b.key; });
    CHECK(all.size() == std::min(n, limit));
    for (size_t i = 0; i < all.size(); ++i) CHECK(all[i].key == rows[i].key && all[i].id == rows[i].id);
    enter(n < limit ? "key_fewer_rows_than_limit" : "key_more_rows_than_limit");
    if (pads_in_the_middle) enter("key_pads_in_the_middle");
    if (holes) enter("key_pads_inside_a_run");
    if (limit == 1) enter("key_limit_1");
    if (empty_shard) enter("key_empty_shard");
}

// ---- by score --------------------------------------------------------------------------------------------------------------------------
void by_score(Rng& rng, size_t G, size_t n, uint32_t limit, uint32_t capacity, std::vector<ShardHit>& scratch) {
    struct Row { float score; uint64_t id; };
    std::vector<Row> rows;                                   // few distinct scores: ties across and inside shards
    for (size_t r = 0; r < n; ++r) rows.push_back(Row{0.25f * (float)upto(rng, 5) - 0.5f, 1000 + 3 * r});
    const auto better = [](const Row& a, const Row& b) { return a.score > b.score; };   // one engine: score descending, row ascending
    const std::vector<size_t> cut = split(rng, n, G);
    std::vector<std::vector<uint64_t>> ids(G);
    std::vector<std::vector<float>> scores(G);
    std::vector<ShardAnswer> parts(G);
    for (size_t g = 0; g < G; ++g) {
        std::vector<Row> mine(rows.begin() + (long)cut[g], rows.begin() + (long)cut[g + 1]);
        std::stable_sort(mine.begin(), mine.end(), better);
        if (mine.size() > limit) mine.resize(limit);
        for (const Row& r : mine) { ids[g].push_back(r.id); scores[g].push_back(r.score); }
        parts[g] = ShardAnswer{ids[g].data(), scores[g].data(), (uint32_t)mine.size()};
    }
    std::vector<uint64_t> out_ids(capacity + 1, 99);
    std::vector<float> out_scores(capacity + 1, 99.f);
    if (!scratch.empty()) enter("score_scratch_reused");
    const uint32_t m = merge_by_score(parts, limit, capacity, out_ids.data(), out_scores.data(), scratch);
    std::vector<Row> model = rows;
    std::stable_sort(model.begin(), model.end(), better);
    CHECK(m == std::min<size_t>(n, std::min(limit, capacity)));
    CHECK(out_ids[m] == 99 && out_scores[m] == 99.f);        // nothing past the count
    bool across = false, inside = false;
    for (uint32_t i = 0; i < m; ++i) {
        CHECK(out_ids[i] == model[i].id && out_scores[i] == model[i].score);
        if (i > 0 && out_scores[i] == out_scores[i - 1]) {
            const size_t r0 = (size_t)(out_ids[i - 1] - 1000) / 3, r1 = (size_t)(out_ids[i] - 1000) / 3;
            CHECK(r0 < r1);                                  // shard, then position
            const size_t g0 = (size_t)(std::upper_bound(cut.begin() + 1, cut.end(), r0) - cut.begin() - 1);
            (r1 < cut[g0 + 1] ? inside : across) = true;
        }
    }
    if (across) enter("score_ties_across_shards");
    if (inside) enter("score_ties_inside_a_shard");
    if (capacity == 0) enter("score_capacity_0");
    else if (capacity < limit && capacity < n) enter("score_capacity_below_limit");
}

// ---- timeline --------------------------------------------------------------------------------------------------------------------------
void timeline(Rng& rng, size_t G, size_t n, size_t limit, size_t capacity, bool newest_first, bool want_ts) {
    struct Row { int64_t ts; uint64_t id; };
    const int64_t kTs[] = {std::numeric_limits<int64_t>::min(), -5, -1, 0, 1, 1700000000000ll, std::numeric_limits<int64_t>::max()};
    std::vector<Row> rows;
    for (size_t r = 0; r < n; ++r) rows.push_back(Row{kTs[upto(rng, 6)], (upto(rng, 1) ? 1ull << 63 : 0ull) + 2 * r + (uint64_t)upto(rng, 1) * 1000000});
    // one engine: timestamp (signed; descending for newest first), then frame id ascending, unsigned
    const auto before = [newest_first](const Row& a, const Row& b) {
        if (a.ts != b.ts) return newest_first ? a.ts > b.ts : a.ts < b.ts;
        return a.id < b.id;
    };
    const std::vector<size_t> cut = split(rng, n, G);
    const size_t stride = limit + upto(rng, 2);
    std::vector<uint64_t> ids(G * stride, 77);
    std::vector<int64_t> ts(G * stride, 77);
    std::vector<uint32_t> counts(G, 0);
    for (size_t g = 0; g < G; ++g) {
        std::vector<Row> mine(rows.begin() + (long)cut[g], rows.begin() + (long)cut[g + 1]);
        std::sort(mine.begin(), mine.end(), before);
        if (mine.size() > limit) mine.resize(limit);
        counts[g] = (uint32_t)mine.size();
        for (size_t i = 0; i < mine.size(); ++i) { ids[g * stride + i] = mine[i].id; ts[g * stride + i] = mine[i].ts; }
    }
    std::vector<uint64_t> out_ids(capacity + 1, 99);
    std::vector<int64_t> out_ts(capacity + 1, 99);
    const uint32_t m = merge_timeline(ids.data(), ts.data(), counts.data(), G, stride, newest_first, limit, capacity, out_ids.data(),
                                      want_ts ? out_ts.data() : nullptr);
    std::vector<Row> model = rows;
    std::sort(model.begin(), model.end(), before);
    CHECK(m == std::min(n, std::min(limit, capacity)));
    CHECK(out_ids[m] == 99 && out_ts[m] == 99);
    bool equal_ts = false, extreme = false, high = false;
    for (uint32_t i = 0; i < m; ++i) {
        CHECK(out_ids[i] == model[i].id);
        if (want_ts) CHECK(out_ts[i] == model[i].ts);
        else CHECK(out_ts[i] == 99);
        if (i > 0 && model[i].ts == model[i - 1].ts) {
            equal_ts = true;
            if (model[i].id >> 63 && !(model[i - 1].id >> 63)) high = true;   // a signed comparison would have put it first
        }
        extreme = extreme || model[i].ts == kTs[0] || model[i].ts == kTs[6];
    }
    enter(newest_first ? "timeline_newest_first" : "timeline_oldest_first");
    if (equal_ts) enter("timeline_equal_timestamps_by_id");
    if (extreme) enter("timeline_extreme_timestamps");
    if (high) enter("timeline_ids_from_2_63");
    if (capacity < limit && capacity < n) enter("timeline_capacity_below_limit");
    if (!want_ts) enter("timeline_without_timestamps_out");
}

// ---- grouped ---------------------------------------------------------------------------------------------------------------------------
constexpr uint64_t kNoMember = ~0ull;

// one engine (or one shard) over rows [lo, hi): per root its best row — the smaller distance bits, the lower row on equal bits —, the roots
// by (bits signed, root id unsigned), the first `limit`
struct GRow { uint64_t root; int64_t dist; };
struct GAnswer { uint64_t root; int64_t dist; size_t row; };
std::vector<GAnswer> grouped_of(const std::vector<GRow>& rows, size_t lo, size_t hi, size_t limit) {
    std::map<uint64_t, GAnswer> best;
    for (size_t r = lo; r < hi; ++r) {
        auto it = best.find(rows[r].root);
        if (it == best.end()) best.emplace(rows[r].root, GAnswer{rows[r].root, rows[r].dist, r});
        else if (rows[r].dist < it->second.dist) it->second = GAnswer{rows[r].root, rows[r].dist, r};
    }
    std::vector<GAnswer> out;
    for (const auto& kv : best) out.push_back(kv.second);
    std::sort(out.begin(), out.end(), [](const GAnswer& a, const GAnswer& b) { return a.dist != b.dist ? a.dist < b.dist : a.root < b.root; });
    if (out.size() > limit) out.resize(limit);
    return out;
}

void grouped(Rng& rng, size_t G, size_t n, size_t limit, size_t n_roots, bool members) {
    std::vector<GRow> rows;                                  // roots on both sides of 2^63; few distinct distances, negative ones among them
    for (size_t r = 0; r < n; ++r) {
        const uint64_t root = upto(rng, n_roots - 1);
        rows.push_back(GRow{(root % 2 ? 1ull << 63 : 0ull) + root, (int64_t)upto(rng, 6) * 1000 - 3000});
    }
    const std::vector<size_t> cut = split(rng, n, G);
    GroupMerge merge;
    std::map<uint64_t, std::vector<int64_t>> offered;        // per root: the bits each shard answered with
    for (size_t g = 0; g < G; ++g)
        for (const GAnswer& a : grouped_of(rows, cut[g], cut[g + 1], limit)) {
            merge.offer(a.root, GroupBest{a.dist, members ? (int64_t)(a.row * 16) : kPad, members ? 5 * a.row + 2 : kNoMember});
            offered[a.root].push_back(a.dist);
        }
    const std::vector<std::pair<int64_t, uint64_t>> got = merge.first(limit);
    const std::vector<GAnswer> model = grouped_of(rows, 0, n, limit);
    CHECK(got.size() == model.size());
    bool different = false, equal = false, negative = false;
    for (size_t i = 0; i < got.size(); ++i) {
        CHECK(got[i].first == model[i].dist && got[i].second == model[i].root);
        const GroupBest& b = merge.best(got[i].second);
        CHECK(b.dist == model[i].dist);
        if (members) CHECK(b.member == 5 * model[i].row + 2 && b.key == (int64_t)(model[i].row * 16));   // the best row's, the lower shard's on equal bits
        else CHECK(b.member == kNoMember && b.key == kPad);
        const std::vector<int64_t>& o = offered[got[i].second];
        const size_t at_best = (size_t)std::count(o.begin(), o.end(), model[i].dist);
        if (o.size() > at_best) different = true;
        if (at_best > 1) equal = true;
        negative = negative || model[i].dist < 0;
    }
    if (different) enter("grouped_root_in_several_shards_different_bits");
    if (equal) enter("grouped_root_in_several_shards_equal_bits");
    if (negative) enter("grouped_negative_bits");
    if (offered.size() > limit) enter("grouped_more_roots_than_limit");
    enter(members ? "grouped_with_members" : "grouped_without_members");
}

}  // namespace

int main() {
    for (const char* s : kStates) g_entered[s] = 0;
    std::vector<ShardHit> scratch;
    for (size_t G = 1; G <= 9; ++G)
        for (unsigned seed = 0; seed < 40; ++seed) {
            Rng rng(100 * G + seed);
            const size_t n = seed % 8 == 0 ? (size_t)upto(rng, 3) : (size_t)upto(rng, 300);
            const size_t limit = seed % 5 == 0 ? 1 : 1 + (size_t)upto(rng, seed % 2 ? 20 : 200);
            by_key(rng, G, n, limit, seed % 4 == 1);
            const uint32_t capacity = seed % 7 == 0 ? 0u : seed % 3 == 0 ? (uint32_t)upto(rng, limit) : (uint32_t)(limit + upto(rng, 5));
            by_score(rng, G, n, (uint32_t)limit, capacity, scratch);
            timeline(rng, G, n, limit, capacity, seed % 2 == 0, seed % 3 != 1);
            grouped(rng, G, n, limit, 1 + (size_t)upto(rng, seed % 2 ? 8 : 60), seed % 4 < 2);
        }
    unsigned long long total = 0;
    for (const auto& kv : g_entered) {
        std::printf("state %s %llu\n", kv.first.c_str(), kv.second);
        total += kv.second;
    }
    CHECK(g_entered.size() == std::size(kStates));
    for (const auto& kv : g_entered) CHECK(kv.second > 0);
    std::printf("ok: shard_merge held to one engine over 1 .. 9 shards, %llu entries of %zu states\n", total, g_entered.size());
    return 0;
}
