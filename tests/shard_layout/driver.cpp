// Stand-alone driver of wax_amd/csrc/shard_layout.h (no HIP, no GPU): the row layout of a sharded handle against a naive model of ONE
// engine — a single vector of ids in insertion order. The shards are plain vectors; every decision (block size, tail shard and room, the
// moves of a doubling, what a reserve asks, the slices of a loaded segment, the bases) comes from the header, and the driver only carries
// it out, as sharded.inc does with engines and peer copies. 1 .. 9 shards, directed cases and seeded random sequences of appends, removals,
// reserves and segment loads; every doubling is also stopped after each of its moves on a copy, where a later append must still land at
// the end. Prints one `state NAME COUNT` line per state and a final `ok:` line; any disagreement prints FAILED and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "shard_layout.h"

namespace {

const char* const kStates[] = {
    "first_batch_below_the_floor_stays_in_shard_0", "min_mb_0_spreads_from_the_first_row", "one_shard_doubles_without_moves",
    "odd_shard_count_doubling", "even_shard_count_doubling", "doubling_stopped_after_every_move", "failed_doubling_then_append",
    "second_doubling_after_a_failed_one", "append_over_several_blocks", "append_after_removal_goes_to_the_tail",
    "reserve_on_an_empty_handle_adopts_the_layout", "reserve_on_a_non_empty_handle_keeps_it", "reserve_hint_sizes_the_first_rows",
    "reserve_covers_the_announced_rows", "segment_shorter_than_one_block", "segment_ends_on_a_block_edge", "segment_with_an_empty_tail_shard",
    "segment_into_a_larger_block", "block_size_rules", "random_sequences",
};
std::map<std::string, unsigned long long> g_entered;
void enter(const std::string& s) { g_entered[s] += 1; }

[[noreturn]] void die(const char* what, int line) {
    std::printf("FAILED: %s (line %d)\n", what, line);
    std::fflush(stdout);
    std::_Exit(1);
}
#define CHECK(c) do { if (!(c)) die(#c, __LINE__); } while (0)

constexpr uint64_t kInitialReserve = 64;

struct Handle {
    ShardLayout::Shape shape;
    ShardLayout layout;
    std::vector<std::vector<uint64_t>> shards;
    std::vector<uint64_t> model;            // one engine: the ids in insertion order
    bool regular = true;                    // no doubling has stopped half way: every shard holds at most block_rows
    bool probe = true;                      // stop every doubling after each of its moves, on a copy
    uint64_t next_id = 1;

    Handle(size_t G, uint32_t dims, int64_t min_mb) : shape{G, dims, min_mb, kInitialReserve}, shards(G) {}
    size_t G() const { return shards.size(); }
    std::vector<uint64_t> counts() const {
        std::vector<uint64_t> c;
        for (const auto& s : shards) c.push_back(s.size());
        return c;
    }
    size_t last_non_empty() const {
        size_t t = 0;
        for (size_t g = 0; g < G(); ++g)
            if (!shards[g].empty()) t = g;
        return t;
    }
    // the concatenation of the shards is the model, and the bases say where each shard's rows begin in it
    void agree() const {
        std::vector<uint64_t> cat;
        for (const auto& s : shards) cat.insert(cat.end(), s.begin(), s.end());
        CHECK(cat == model);
        const std::vector<uint64_t> c = counts(), bases = ShardLayout::bases(c.data(), G());
        CHECK(bases.size() == G() && bases[0] == 0);
        for (size_t g = 0; g < G(); ++g) {
            CHECK(bases[g] <= model.size());
            if (!shards[g].empty()) CHECK(model[bases[g]] == shards[g][0]);
            if (g + 1 < G()) CHECK(bases[g + 1] == bases[g] + c[g]);
        }
    }
    void within_blocks() const {
        if (regular)
            for (const auto& s : shards) CHECK(s.size() <= layout.block_rows);
    }
    static void move_all(std::vector<std::vector<uint64_t>>& sh, size_t src, size_t dst) {
        sh[dst].insert(sh[dst].end(), sh[src].begin(), sh[src].end());
        sh[src].clear();
    }

    // false: the doubling stopped before its move number `fail_at` (an engine's failed peer copy), the block size as it was
    bool double_blocks(long fail_at) {
        const std::vector<std::pair<size_t, size_t>> moves = ShardLayout::doubling_moves(G());
        CHECK(moves.size() == G() - 1);
        if (probe && model.size() <= 4096) {
            for (size_t j = 0; j <= moves.size(); ++j) {          // (j = all of them: the block size still as it was)
                Handle h = *this;
                h.probe = false;
                for (size_t i = 0; i < j; ++i) move_all(h.shards, moves[i].first, moves[i].second);
                h.regular = false;
                h.agree();
                CHECK(h.append(1 + j % 3));
                CHECK(h.append(layout.block_rows + 1));
            }
            enter("doubling_stopped_after_every_move");
        }
        const std::vector<uint64_t> before = counts();
        const uint64_t block_before = layout.block_rows;
        std::vector<bool> read(G(), false);
        std::vector<uint64_t> moved_in(G(), 0);
        for (size_t j = 0; j < moves.size(); ++j) {
            if ((long)j == fail_at) {
                if (j > 0) regular = false;
                CHECK(layout.block_rows == block_before);
                return false;
            }
            const size_t src = moves[j].first, dst = moves[j].second;
            CHECK(src < G() && dst < src && !read[src]);
            // no source is overwritten before it is read: the target was emptied as a source earlier in this pass and holds nothing but
            // what this pass has moved into it since — or it is shard 0, which keeps its rows and takes shard 1's
            if (dst == 0) CHECK(src == 1);
            else CHECK(read[dst] && shards[dst].size() == moved_in[dst]);
            moved_in[dst] += shards[src].size();
            move_all(shards, src, dst);
            read[src] = true;
            agree();                                                          // order is kept after every move
        }
        for (size_t g = 1; g < G(); ++g) CHECK(read[g]);
        layout.doubled();
        CHECK(layout.block_rows == 2 * block_before);
        for (size_t h = 0; h < G(); ++h) {
            const uint64_t want = (2 * h < G() ? before[2 * h] : 0) + (2 * h + 1 < G() ? before[2 * h + 1] : 0);
            CHECK(shards[h].size() == want);
        }
        within_blocks();
        if (!regular) enter("second_doubling_after_a_failed_one");
        enter(G() % 2 ? "odd_shard_count_doubling" : "even_shard_count_doubling");
        return true;
    }

    // n new rows at the end, as sh_add_batch_device places them. false: a doubling failed; the rows placed before it stay.
    bool append(uint64_t n, long fail_at = -1) {
        layout.first_rows(shape, n);
        CHECK(layout.block_rows >= kInitialReserve && layout.block_rows % 64 == 0);
        uint64_t i = 0, chunks = 0;
        while (i < n) {
            size_t t = 0;
            uint64_t room = 0;
            for (;;) {
                const std::vector<uint64_t> c = counts();
                const uint64_t block_before = layout.block_rows;
                if (layout.tail(c.data(), G(), &t, &room)) {
                    if (layout.block_rows != block_before) {
                        CHECK(G() == 1 && layout.block_rows > c[0] && layout.block_rows / 2 <= c[0]);
                        enter("one_shard_doubles_without_moves");
                    }
                    break;
                }
                CHECK(G() > 1 && layout.block_rows == block_before);
                CHECK(c[G() - 1] >= layout.block_rows);                      // "all full": the last shard is
                if (!double_blocks(fail_at)) {
                    agree();
                    return false;
                }
                fail_at = -1;
            }
            const size_t last = last_non_empty();
            CHECK(room > 0 && shards[t].size() + room == layout.block_rows);
            CHECK(t == last || (t == last + 1 && shards[last].size() >= layout.block_rows));   // the last shard with rows, or the one behind it
            if (model.empty()) CHECK(t == 0);
            const uint64_t m = std::min(room, n - i);
            for (uint64_t j = 0; j < m; ++j) {
                shards[t].push_back(next_id);
                model.push_back(next_id++);
            }
            i += m;
            ++chunks;
            within_blocks();
            agree();
        }
        if (chunks >= 3) enter("append_over_several_blocks");
        return true;
    }

    void remove_row(uint64_t row) {
        const std::vector<uint64_t> c = counts(), bases = ShardLayout::bases(c.data(), G());
        size_t g = 0;
        while (!(row >= bases[g] && row < bases[g] + c[g])) ++g;
        shards[g].erase(shards[g].begin() + (long)(row - bases[g]));
        model.erase(model.begin() + (long)row);
        agree();
    }

    std::vector<uint64_t> reserve(uint64_t rows) {
        const uint64_t held = model.size(), block_before = layout.block_rows, hint_before = layout.reserve_hint;
        const std::vector<uint64_t> ask = layout.reserve(shape, rows, counts().data());
        CHECK(layout.reserve_hint == std::max(hint_before, rows));
        const uint64_t per = ShardLayout::block_rows_for(shape, rows);
        if (held == 0) { CHECK(layout.block_rows == per); enter("reserve_on_an_empty_handle_adopts_the_layout"); }
        else { CHECK(layout.block_rows == block_before); enter("reserve_on_a_non_empty_handle_keeps_it"); }
        // shards fill in order, in blocks of the larger of the two sizes
        const uint64_t blk = std::max(per, layout.block_rows);
        uint64_t left = std::max(rows, held);
        CHECK(ask.size() == G());
        for (size_t g = 0; g < G(); ++g) {
            CHECK(ask[g] == std::min(left, blk));
            left -= ask[g];
        }
        if (regular) CHECK(left == 0);                                       // (blocks that a stopped doubling left over-full hold more than G blocks)
        return ask;
    }

    void load(uint64_t n) {
        const uint64_t block_before = layout.block_rows;
        std::vector<uint64_t> ids;
        for (uint64_t i = 0; i < n; ++i) ids.push_back(next_id++);
        layout.segment(shape, n);
        CHECK(layout.block_rows >= block_before && layout.block_rows >= ShardLayout::block_rows_for(shape, n));
        uint64_t at = 0;
        for (size_t g = 0; g < G(); ++g) {
            uint64_t lo = 0, hi = 0;
            layout.slice(g, n, &lo, &hi);
            CHECK(lo == at && hi >= lo && hi <= n && hi - lo <= layout.block_rows);
            if (hi < n) CHECK(hi - lo == layout.block_rows);                 // only the last shard with rows is short
            shards[g].assign(ids.begin() + (long)lo, ids.begin() + (long)hi);
            at = hi;
        }
        CHECK(at == n);
        model = ids;
        regular = true;
        within_blocks();
        agree();
        if (n > 0 && n < layout.block_rows) { CHECK(shards[0].size() == n); enter("segment_shorter_than_one_block"); }
        if (n > 0 && n % layout.block_rows == 0) enter("segment_ends_on_a_block_edge");
        if (n > 0 && G() > 1 && shards[G() - 1].empty()) enter("segment_with_an_empty_tail_shard");
        if (block_before > ShardLayout::block_rows_for(shape, n)) { CHECK(layout.block_rows == block_before); enter("segment_into_a_larger_block"); }
    }
};

// ---- directed cases ------------------------------------------------------------------------------------------------------------------
void block_size_rules() {
    using S = ShardLayout::Shape;
    CHECK(ShardLayout::block_rows_for(S{3, 256, 0, 64}, 3000) == 1024);      // ceil(3000 / 3) = 1000 -> 1024
    CHECK(ShardLayout::block_rows_for(S{3, 256, 0, 64}, 3072) == 1024);
    CHECK(ShardLayout::block_rows_for(S{3, 256, 0, 64}, 3073) == 1088);
    CHECK(ShardLayout::block_rows_for(S{3, 256, 0, 64}, 100) == 64);         // ceil(100 / 3) = 34 -> 64
    CHECK(ShardLayout::block_rows_for(S{3, 256, 0, 64}, 0) == 64);           // never below the initial reservation
    CHECK(ShardLayout::block_rows_for(S{4, 64, 0, 1024}, 100) == 1024);
    CHECK(ShardLayout::block_rows_for(S{2, 256, 1, 64}, 10) == 1024);        // 1 MB of 1 KB rows
    CHECK(ShardLayout::block_rows_for(S{2, 256, 1, 64}, 4096) == 2048);      // the floor is a floor
    CHECK(ShardLayout::block_rows_for(S{2, 100, 1, 64}, 10) == 2624);        // 1 MB / 400 B = 2621.44 -> 2622 -> 2624
    CHECK(ShardLayout::block_rows_for(S{1, 256, 64, 64}, 10) == 64);         // one shard: no floor
    CHECK(ShardLayout::block_rows_for(S{8, 384, 64, 64}, 1000000) == 125056);
    CHECK(ShardLayout::block_rows_for(S{8, 384, 64, 64}, 100000) == 43712);  // 64 MB / 1536 B = 43690.67 -> 43691 -> 43712
    CHECK(ShardLayout::round_up64(0) == 0 && ShardLayout::round_up64(1) == 64 && ShardLayout::round_up64(64) == 64 && ShardLayout::round_up64(65) == 128);
    enter("block_size_rules");
}

void small_store_rule() {
    for (size_t G = 2; G <= 9; ++G) {
        Handle h(G, 256, 1);                                                 // the floor: 1 024 rows
        CHECK(h.append(10));
        CHECK(h.layout.block_rows == 1024 && h.shards[0].size() == 10);
        CHECK(h.append(1014));
        CHECK(h.shards[0].size() == 1024 && h.shards[1].empty());
        enter("first_batch_below_the_floor_stays_in_shard_0");
        CHECK(h.append(1));
        CHECK(h.shards[0].size() == 1024 && h.shards[1].size() == 1);
        Handle z(G, 256, 0);
        CHECK(z.append(200));                                                // ceil(200 / G) -> 64 or 128 rows per block
        CHECK(z.layout.block_rows == (G < 4 ? 128u : 64u) && z.shards[0].size() == z.layout.block_rows && !z.shards[1].empty());
        enter("min_mb_0_spreads_from_the_first_row");
    }
}

void reserve_cases() {
    for (size_t G = 1; G <= 9; ++G) {
        Handle h(G, 256, 0);
        const std::vector<uint64_t> ask = h.reserve(3000);                   // before the first rows
        CHECK(h.layout.block_rows == ShardLayout::round_up64((3000 + G - 1) / G));
        for (int i = 0; i < 30; ++i) {
            CHECK(h.append(100));
            for (size_t g = 0; g < G; ++g) CHECK(h.shards[g].size() <= ask[g]);   // what was reserved is what the rows occupy
        }
        enter("reserve_covers_the_announced_rows");
        (void)h.reserve(100);                                                // after: the layout stays, every held row is covered
        (void)h.reserve(50000);
        Handle f(G, 256, 0);                                                 // a hint, then a setting that makes an empty handle choose again
        (void)f.reserve(6400);
        f.layout.block_rows = 0;
        CHECK(f.append(1));
        CHECK(f.layout.block_rows == ShardLayout::block_rows_for(f.shape, 6400) && f.layout.block_rows >= 6400 / G);
        enter("reserve_hint_sizes_the_first_rows");
    }
}

void segment_cases() {
    for (size_t G = 1; G <= 9; ++G) {
        { Handle h(G, 256, 1); h.load(700); if (G > 1) CHECK(h.shards[0].size() == 700); CHECK(h.append(400)); }   // below the floor: shard 0 alone
        { Handle h(G, 256, 0); h.load(64 * G); CHECK(h.layout.block_rows == 64 && h.shards[G - 1].size() == 64); CHECK(h.append(5)); }
        { Handle h(G, 256, 0); h.load(64 * G - 64 + (G == 1 ? 64 : 0)); CHECK(h.append(70)); }
        { Handle h(G, 256, 0); h.load(64 * G + 1); CHECK(h.layout.block_rows == 128); CHECK(h.append(1000)); }
        { Handle h(G, 256, 0); (void)h.reserve(1280 * G); h.load(300); CHECK(h.layout.block_rows == 1280 && h.shards[0].size() == 300); }
        { Handle h(G, 256, 0); h.load(0); CHECK(h.append(3)); }
    }
}

void failed_doubling() {
    for (size_t G = 2; G <= 9; ++G)
        for (long fail_at = 0; fail_at < (long)G - 1; ++fail_at) {
            Handle h(G, 256, 0);
            CHECK(h.append(64 * G));                                         // every shard full at 64 rows
            CHECK(!h.append(10, fail_at));                                   // the doubling stops before move `fail_at`
            CHECK(h.layout.block_rows == 64 && h.model.size() == 64 * G);
            CHECK(h.append(10));                                             // the next append finds the end (doubling again if it must)
            CHECK(h.append(64 * G));
            h.remove_row(0);
            CHECK(h.append(300));
            enter("failed_doubling_then_append");
        }
}

void removal_then_append() {
    for (size_t G = 2; G <= 9; ++G) {
        Handle h(G, 256, 0);
        CHECK(h.append(64 * 2 + 5));
        for (int i = 0; i < 20; ++i) h.remove_row(3);                        // room in shard 0: new rows still go to the tail
        const size_t tail = h.last_non_empty();
        const uint64_t before = h.shards[0].size();
        CHECK(h.append(7));
        CHECK(h.shards[0].size() == before && h.last_non_empty() == tail);
        enter("append_after_removal_goes_to_the_tail");
    }
}

void random_sequences() {
    for (size_t G = 1; G <= 9; ++G)
        for (int64_t min_mb = 0; min_mb <= 1; ++min_mb)
            for (unsigned seed = 0; seed < 3; ++seed) {
                std::mt19937_64 rng(1000 * G + 10 * seed + (unsigned)min_mb);
                auto upto = [&rng](uint64_t n) { return (uint64_t)(rng() % (n + 1)); };
                Handle h(G, 4096, min_mb);                                   // the floor: 64 rows
                if (seed % 2) (void)h.reserve(upto(3000));
                for (int step = 0; step < 40; ++step) {
                    const uint64_t op = upto(9), block = std::max<uint64_t>(h.layout.block_rows, 64);
                    if (op <= 4) {
                        const uint64_t n = 1 + upto(op == 0 ? 3 * block : op == 1 ? block : 40);
                        const long fail_at = G > 1 && upto(7) == 0 ? (long)upto(G - 2) : -1;
                        (void)h.append(n, fail_at);
                    } else if (op <= 6) {
                        for (uint64_t r = upto(30); r > 0 && !h.model.empty(); --r) h.remove_row(upto(h.model.size() - 1));
                    } else if (op == 7) {
                        (void)h.reserve(upto(4 * block * G));
                    } else if (op == 8 && upto(2) == 0) {
                        h.load(upto(2) == 0 ? block * (1 + upto(G - 1)) : upto(2 * block * G));
                    }
                }
                CHECK(h.append(1));
                enter("random_sequences");
            }
}

}  // namespace

int main() {
    for (const char* s : kStates) g_entered[s] = 0;
    block_size_rules();
    small_store_rule();
    reserve_cases();
    segment_cases();
    failed_doubling();
    removal_then_append();
    random_sequences();
    unsigned long long total = 0;
    for (const auto& kv : g_entered) {
        std::printf("state %s %llu\n", kv.first.c_str(), kv.second);
        total += kv.second;
    }
    CHECK(g_entered.size() == std::size(kStates));
    for (const auto& kv : g_entered) CHECK(kv.second > 0);
    std::printf("ok: shard_layout held to one vector of ids over 1 .. 9 shards, %llu entries of %zu states\n", total, g_entered.size());
    return 0;
}
