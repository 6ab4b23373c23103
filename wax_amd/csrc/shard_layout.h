// shard_layout.h — where the rows of a sharded handle live: contiguous row blocks, shard g holding global rows
// [base_g, base_g + count_g), so that the concatenation of the shards IS one engine's row order. Plain C++17 over the standard library:
// no HIP, no project header, and no engine — the per-shard row counts go in as a plain array. sharded.inc carries the decisions out
// (peer copies, the shards' own add / reserve / deserialize); tests/shard_layout/driver.cpp carries them out on plain vectors and holds
// the result to ONE vector of ids in insertion order, for 1 .. 9 shards.
//
//   decision                     rule
//   block_rows_for(want)         ceil(want / G) rounded up to 64 rows, never below `initial_reserve`; with more than one shard never
//                                below `min_mb` MB of rows either (the small-store rule: a store under one block lives on shard 0)
//   first_rows(n)                no block size chosen yet: the one for max(reserve_hint, n) rows
//   tail(counts)                 the last shard that holds rows, or the one behind it when that one is full; its room. All full: one
//                                shard doubles its block there and then (the block size is only a formality), more shards say so and
//                                the caller performs doubling_moves()
//   doubling_moves()             new shard h = old shards 2h, 2h + 1 in order, as (source, target) moves of ALL rows of the source to
//                                the END of the target, in the order to perform them. In place: target h > 0 was emptied when it served
//                                as a source of an earlier target (h = 2h' or 2h' + 1 with h' < h), sources 2h, 2h + 1 >= h are not yet
//                                overwritten; target 0 keeps its rows and takes shard 1's. Stopping after ANY prefix of the moves leaves
//                                every row where the concatenation still is the global order, and tail() (counts only) still finds the
//                                end. doubled() after the full pass: the block size is twice what it was
//   reserve(rows, counts)        the hint grows to `rows`; an empty handle adopts block_rows_for(rows); shards fill in order, so shard g
//                                is asked for what max(rows, held) rows occupy of it in blocks of max(that, block_rows) — 0 from the
//                                first shard that stays empty on
//   segment(n) / slice(g, n)     a loaded segment of n rows: the block is at least block_rows_for(n), and shard g loads rows
//                                [min(n, g * block), min(n, (g + 1) * block))
//   bases(counts)                base_g = the sum of the counts before it
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

struct ShardLayout {
    // what the block size depends on besides the rows announced
    struct Shape {
        size_t shards;              // G
        uint32_t dims;
        int64_t min_mb;             // "shard_min_mb" (0 = spread from the first row)
        uint64_t initial_reserve;   // a single engine's first reservation
    };

    uint64_t block_rows = 0;        // rows at which a shard is full (0 = not chosen yet)
    uint64_t reserve_hint = 0;

    static uint64_t round_up64(uint64_t x) { return (x + 63ull) & ~63ull; }

    static uint64_t block_rows_for(const Shape& sh, uint64_t want) {
        const uint64_t G = sh.shards, row_bytes = (uint64_t)sh.dims * 4;
        uint64_t per = std::max<uint64_t>(sh.initial_reserve, round_up64((want + G - 1) / G));
        if (sh.min_mb > 0 && G > 1) per = std::max<uint64_t>(per, round_up64((((uint64_t)sh.min_mb << 20) + row_bytes - 1) / row_bytes));
        return per;
    }

    void first_rows(const Shape& sh, uint64_t n) {
        if (block_rows == 0) block_rows = block_rows_for(sh, std::max<uint64_t>(reserve_hint, n));
    }

    // false: every shard is full (more than one shard: perform doubling_moves(), then doubled(), and ask again)
    bool tail(const uint64_t* counts, size_t G, size_t* shard, uint64_t* room) {
        size_t t = 0;
        for (size_t g = 0; g < G; ++g)
            if (counts[g] > 0) t = g;
        if (counts[t] >= block_rows && t + 1 < G) ++t;
        if (G == 1)
            while (counts[t] >= block_rows) block_rows *= 2;
        if (counts[t] >= block_rows) return false;
        *shard = t;
        *room = block_rows - counts[t];
        return true;
    }

    static std::vector<std::pair<size_t, size_t>> doubling_moves(size_t G) {
        std::vector<std::pair<size_t, size_t>> moves;
        for (size_t h = 0; 2 * h < G; ++h)
            for (size_t src = 2 * h; src <= 2 * h + 1 && src < G; ++src)
                if (src != h) moves.emplace_back(src, h);   // (h = 0: shard 0 keeps its rows, shard 1 is appended)
        return moves;
    }
    void doubled() { block_rows *= 2; }

    // rows to reserve on each shard
    std::vector<uint64_t> reserve(const Shape& sh, uint64_t rows, const uint64_t* counts) {
        uint64_t held = 0;
        for (size_t g = 0; g < sh.shards; ++g) held += counts[g];
        reserve_hint = std::max(reserve_hint, rows);
        const uint64_t per = block_rows_for(sh, rows);
        if (held == 0) block_rows = per;
        const uint64_t blk = std::max(per, block_rows);
        std::vector<uint64_t> ask(sh.shards, 0);
        uint64_t left = std::max(rows, held);
        for (size_t g = 0; g < sh.shards; ++g) {
            ask[g] = std::min(left, blk);
            left -= ask[g];
        }
        return ask;
    }

    void segment(const Shape& sh, uint64_t n) { block_rows = std::max(block_rows_for(sh, n), block_rows); }
    void slice(size_t g, uint64_t n, uint64_t* lo, uint64_t* hi) const {
        *lo = std::min<uint64_t>(n, g * block_rows);
        *hi = std::min<uint64_t>(n, (g + 1) * block_rows);
    }

    static std::vector<uint64_t> bases(const uint64_t* counts, size_t G) {
        std::vector<uint64_t> out(G);
        uint64_t base = 0;
        for (size_t g = 0; g < G; ++g) {
            out[g] = base;
            base += counts[g];
        }
        return out;
    }
};
