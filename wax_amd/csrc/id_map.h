// id_map.h — frameId -> row on the host. Plain C++17 over the standard library: no HIP and no project header;
// tests/id_map/driver.cpp holds it to std::unordered_map on the CPU, probe clusters that wrap round the end of the table included.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

// frameId -> row. Open addressing, linear probing, backward-shift deletion. Replaces the
// reference's O(N) `frameIds.firstIndex(of:)` (MetalVectorEngine.swift:334, 385, 426).
class IdMap {
  public:
    IdMap() { resize_table(1024); }
    int64_t find(uint64_t id) const {
        size_t i = hash(id) & mask_;
        while (used_[i]) {
            if (keys_[i] == id) return (int64_t)vals_[i];
            i = (i + 1) & mask_;
        }
        return -1;
    }
    void put(uint64_t id, uint32_t row) {
        if ((size_ + 1) * 10 > (mask_ + 1) * 6) grow();
        size_t i = hash(id) & mask_;
        while (used_[i]) {
            if (keys_[i] == id) { vals_[i] = row; return; }
            i = (i + 1) & mask_;
        }
        used_[i] = 1; keys_[i] = id; vals_[i] = row; ++size_;
    }
    // remove `id` (stored at row `row`) and renumber every row above it down by one
    void erase_row(uint64_t id, uint32_t row) {
        erase_only(id);
        for (size_t s = 0; s <= mask_; ++s)
            if (used_[s] && vals_[s] > row) --vals_[s];
    }
    // After erase_only of the ids of the rows `rem` (ascending, distinct): every remaining row drops by the number of removed rows
    // below it, in ONE pass over the table (n calls of erase_row are n passes). rank(r) comes from a bitmap of the removed rows
    // with a running count per 64-row word — 1 bit + half a byte per 64 rows behind rem[0], cache-resident at 10M rows.
    void renumber_removed(const std::vector<uint32_t>& rem, uint64_t rows) {
        if (rem.empty()) return;
        const uint64_t first = rem[0] & ~63ull;                    // word-aligned start of the affected range
        const size_t words = (size_t)((rows - first + 63) / 64);
        std::vector<uint64_t> bits(words, 0);
        std::vector<uint32_t> before(words, 0);                    // removed rows below the word
        for (uint32_t r : rem) bits[(r - first) >> 6] |= 1ull << ((r - first) & 63);
        uint32_t run = 0;
        for (size_t w = 0; w < words; ++w) { before[w] = run; run += (uint32_t)__builtin_popcountll(bits[w]); }
        for (size_t s = 0; s <= mask_; ++s) {
            if (!used_[s] || vals_[s] <= rem[0]) continue;
            const uint64_t o = vals_[s] - first;
            vals_[s] -= before[o >> 6] + (uint32_t)__builtin_popcountll(bits[o >> 6] & ((1ull << (o & 63)) - 1ull));
        }
    }
    void erase_only(uint64_t id) {
        size_t i = hash(id) & mask_;
        while (used_[i] && keys_[i] != id) i = (i + 1) & mask_;
        if (used_[i]) {
            size_t hole = i, j = i;
            for (;;) {
                j = (j + 1) & mask_;
                if (!used_[j]) break;
                const size_t home = hash(keys_[j]) & mask_;
                // can entry j move into the hole? yes iff hole lies cyclically in [home, j)
                const bool movable = (hole <= j) ? (home <= hole || home > j) : (home <= hole && home > j);
                if (movable) {
                    keys_[hole] = keys_[j]; vals_[hole] = vals_[j];
                    hole = j;
                }
            }
            used_[hole] = 0;
            --size_;
        }
    }
    void clear() { resize_table(1024); }
    void reserve(size_t n) {
        size_t want = 1024;
        while (want * 6 < n * 10 + 10) want <<= 1;
        if (want > mask_ + 1) rehash(want);
    }
    size_t size() const { return size_; }
    // for a test that aims at table positions: an id's home slot is hash(id) & (slots() - 1)
    size_t slots() const { return mask_ + 1; }
    static uint64_t hash(uint64_t x) {
        x += 0x9e3779b97f4a7c15ull;
        x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
        x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
        return x ^ (x >> 31);
    }

  private:
    void resize_table(size_t cap) {
        keys_.assign(cap, 0); vals_.assign(cap, 0); used_.assign(cap, 0);
        mask_ = cap - 1; size_ = 0;
    }
    void rehash(size_t cap) {
        std::vector<uint64_t> ok; std::vector<uint32_t> ov; std::vector<uint8_t> ou;
        ok.swap(keys_); ov.swap(vals_); ou.swap(used_);
        resize_table(cap);
        for (size_t s = 0; s < ou.size(); ++s)
            if (ou[s]) put(ok[s], ov[s]);
    }
    void grow() { rehash((mask_ + 1) * 2); }
    std::vector<uint64_t> keys_;
    std::vector<uint32_t> vals_;
    std::vector<uint8_t> used_;
    size_t mask_ = 0, size_ = 0;
};
