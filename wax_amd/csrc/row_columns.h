// row_columns.h — the per-row columns beside the store, on the host: timestamps, flags, parents and term sets.
// Plain C++17 over the standard library and include/wax_hip.h: no HIP, so tests/row_columns/driver.cpp holds it to a naive model on
// the CPU. The engine (engine_types.inc) keeps one RowColumns and, beside it, only what lives on the device: pointers, capacities,
// the mutexes of the three readers and their counters.
//
// The rules every column follows:
//   - the host copy is authoritative and in row order, beside the frame ids; writers change it under the exclusive engine lock;
//   - it may be SHORTER than the store: rows at or behind its end hold the default (what every appended row holds), so the append
//     paths never touch it;
//   - it is empty on a store that never had the column, and a column emptied by removals is such a column again;
//   - a device copy is current for rows [0, dev_rows) below stale_from (UploadMark). Writers only lower the mark; the next reader
//     (ensure_attrs, ensure_groups, ensure_terms) uploads rows [from(count), count) and settles it.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <utility>
#include <vector>

#include "wax_hip.h"

// What a device copy of a column still has to receive. "Nothing on the device" is (0 rows, nothing stale): the state a mark starts in
// and reset() returns to.
class UploadMark {
public:
    static constexpr uint64_t kNone = UINT64_MAX;
    void note(uint64_t row) { stale_from_ = std::min(stale_from_, row); }          // row `row` and the rows behind it may differ now
    uint64_t from(uint64_t count) const { return std::min(std::min(dev_rows_, stale_from_), count); }
    bool current(uint64_t count) const { return dev_rows_ == count && stale_from_ == kNone; }
    void settle(uint64_t count) { dev_rows_ = count; stale_from_ = kNone; }        // a reader has uploaded [from(count), count)
    void reset() { dev_rows_ = 0; stale_from_ = kNone; }
private:
    uint64_t dev_rows_ = 0;
    uint64_t stale_from_ = kNone;                 // lowest row whose device copy may differ from the host's
};

// One value per row.
template <typename T>
class DenseColumn {
public:
    explicit DenseColumn(T dflt) : dflt_(dflt) {}
    uint64_t rows() const { return v_.size(); }
    bool empty() const { return v_.empty(); }
    const T* data() const { return v_.data(); }
    T at(uint64_t row) const { return row < v_.size() ? v_[(size_t)row] : dflt_; }
    // a column that ends at or below `row` first reaches to `count`: everything up to there held the default
    void cover(uint64_t row, uint64_t count) { if (v_.size() <= row) v_.resize((size_t)count, dflt_); }
    void set(uint64_t row, uint64_t count, T v) { cover(row, count); v_[(size_t)row] = v; }
    void erase(uint64_t row) { if (row < v_.size()) v_.erase(v_.begin() + (ptrdiff_t)row); }
    // rows rem[0 .. m) (ascending, unique) leave in one pass from the lowest of them; rows behind the column cost nothing
    template <typename Row>
    void erase_rows(const Row* rem, size_t m) {
        if (m == 0 || (uint64_t)rem[0] >= v_.size()) return;
        size_t w = (size_t)rem[0], p = 0;
        for (size_t r = w; r < v_.size(); ++r) {
            if (p < m && (uint64_t)rem[p] == r) { ++p; continue; }
            v_[w++] = v_[r];
        }
        v_.resize(w);
    }
    // src's rows become rows dst_before .. of this column (which ends at or below dst_before): padded with the default up to there
    void append(const DenseColumn& src, uint64_t dst_before) {
        v_.resize((size_t)dst_before, dflt_);
        v_.insert(v_.end(), src.v_.begin(), src.v_.end());
    }
    void truncate(uint64_t rows) { if (v_.size() > rows) v_.resize((size_t)rows); }
    void clear() { v_.clear(); }
private:
    T dflt_;
    std::vector<T> v_;
};

// One set_terms call, checked against itself (validate_term_sets, api_terms.inc): entry i's distinct terms, ascending, are
// flat[e_off[i] .. e_off[i + 1]) — one allocation for the whole call, sorted and de-duplicated in place.
struct TermPlan {
    std::vector<uint32_t> flat;
    std::vector<uint64_t> e_off;
    uint32_t len(uint64_t entry) const { return (uint32_t)(e_off[(size_t)entry + 1] - e_off[(size_t)entry]); }
    const uint32_t* begin(uint64_t entry) const { return flat.data() + e_off[(size_t)entry]; }
};
// One store's share of a plan: (row, entry) by ascending row, one per row.
typedef std::vector<std::pair<uint64_t, uint64_t>> TermRows;

// (row, entry) pairs in call order -> one per row, ascending, the last entry of a row kept (the last entry of a repeated id wins)
inline void finish_term_rows(TermRows* rows) {
    std::stable_sort(rows->begin(), rows->end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    size_t w = 0;
    for (size_t i = 0; i < rows->size(); ++i)
        if (i + 1 == rows->size() || (*rows)[i + 1].first != (*rows)[i].first) (*rows)[w++] = (*rows)[i];
    rows->resize(w);
}

// A set of 0 .. WAX_HIP_TERMS_MAX_PER_ROW distinct uint32 terms per row, ascending, as CSR: off[r] .. off[r + 1] index row r's terms
// in one flat array, so the offsets are one more than the rows covered. Both arrays are empty on a store without terms; a column
// that covers no row is such a column. The total stays below 2^32: the callers compare total_after / can_append before they write.
class TermColumn {
public:
    struct Span {
        const uint32_t* begin;
        const uint32_t* end;
        uint32_t size() const { return (uint32_t)(end - begin); }
    };
    bool empty() const { return off_.empty(); }
    uint64_t rows() const { return off_.empty() ? 0 : off_.size() - 1; }
    uint64_t total() const { return off_.empty() ? 0 : off_.back(); }
    const uint32_t* values() const { return val_.data(); }
    // where row r's terms begin; the column's end for r at or behind it (the device copy holds count + 1 offsets). Not on an empty column.
    uint32_t offset(uint64_t r) const { return off_[(size_t)std::min<uint64_t>(r, off_.size() - 1)]; }
    Span span(uint64_t r) const {                                   // behind the column: the empty set
        if (r >= rows()) return Span{val_.data(), val_.data()};
        return Span{val_.data() + off_[(size_t)r], val_.data() + off_[(size_t)r + 1]};
    }

    // The terms the column would hold once `rows` of the plan are applied.
    uint64_t total_after(const TermPlan& p, const TermRows& rows) const {
        uint64_t total = this->total();
        for (const auto& re : rows) total = total - span(re.first).size() + p.len(re.second);
        return total;
    }
    // Apply (total_after(p, rows) < 2^32; rows not empty). Sets of the size they had are overwritten in place; otherwise the CSR is
    // rebuilt from the lowest row whose size changes, to the end of the column: the old one's, or the highest row set if that lies
    // behind it — the rows behind the column hold the empty set and need no entry.
    void commit(const TermPlan& p, const TermRows& rows) {
        const uint64_t old_rows = this->rows();
        size_t first_resized = rows.size();
        for (size_t i = 0; i < rows.size(); ++i) {
            const uint32_t len = p.len(rows[i].second);
            if (rows[i].first < old_rows && len == span(rows[i].first).size()) {
                if (len != 0) std::memcpy(val_.data() + off_[(size_t)rows[i].first], p.begin(rows[i].second), (size_t)len * sizeof(uint32_t));
            } else if (first_resized == rows.size()) {
                first_resized = i;
            }
        }
        if (first_resized == rows.size()) return;
        const uint64_t lowest = rows[first_resized].first;
        const uint64_t new_rows = std::max(old_rows, rows.back().first + 1);
        if (off_.empty()) off_.push_back(0u);
        const uint64_t keep_rows = std::min(lowest, old_rows);
        const uint32_t keep = off_[(size_t)keep_rows];
        std::vector<uint32_t> tail_off, tail_val;
        tail_off.reserve((size_t)(new_rows - lowest));
        size_t i = first_resized;
        for (uint64_t r = lowest; r < new_rows; ++r) {
            if (i < rows.size() && rows[i].first == r) {
                tail_val.insert(tail_val.end(), p.begin(rows[i].second), p.begin(rows[i].second) + p.len(rows[i].second));
                ++i;
            } else if (r < old_rows) {
                tail_val.insert(tail_val.end(), val_.begin() + off_[(size_t)r], val_.begin() + off_[(size_t)r + 1]);
            }
            tail_off.push_back(keep + (uint32_t)tail_val.size());
        }
        off_.resize((size_t)keep_rows + 1);
        off_.resize((size_t)lowest + 1, keep);                      // rows between the old column's end and `lowest` held the empty set
        off_.insert(off_.end(), tail_off.begin(), tail_off.end());
        val_.resize((size_t)keep);
        val_.insert(val_.end(), tail_val.begin(), tail_val.end());
    }

    // rows rem[0 .. m) (ascending, unique) leave with their sets: one compaction pass from the lowest of them
    template <typename Row>
    void erase_rows(const Row* rem, size_t m) {
        const uint64_t nt = rows();
        if (m == 0 || (uint64_t)rem[0] >= nt) return;
        uint64_t wr = rem[0];
        uint32_t wv = off_[(size_t)rem[0]], b = wv;
        size_t p = 0;
        for (uint64_t r = rem[0]; r < nt; ++r) {
            const uint32_t en = off_[(size_t)r + 1];
            if (p < m && (uint64_t)rem[p] == r) { ++p; b = en; continue; }
            if (wv != b) std::memmove(val_.data() + wv, val_.data() + b, (size_t)(en - b) * sizeof(uint32_t));
            wv += en - b;
            b = en;
            off_[(size_t)++wr] = wv;                                // (wr <= r + 1: an entry already read, or the one just read with its own value)
        }
        cut(wr, wv);
    }
    void erase(uint64_t row) { erase_rows(&row, 1); }
    bool can_append(const TermColumn& src) const { return src.total() + total() < 0x100000000ull; }
    // src's rows become rows dst_before .. of this column (which ends at or below dst_before): the rows up to there hold what they held
    void append(const TermColumn& src, uint64_t dst_before) {
        if (src.empty()) return;
        if (off_.empty()) off_.push_back(0u);
        off_.resize((size_t)dst_before + 1, off_.back());
        const uint32_t base = off_.back();
        for (size_t r = 1; r < src.off_.size(); ++r) off_.push_back(base + src.off_[r]);
        val_.insert(val_.end(), src.val_.begin(), src.val_.end());
    }
    void truncate(uint64_t rows) { if (this->rows() > rows) cut(rows, off_[(size_t)rows]); }
    void clear() { off_.clear(); val_.clear(); }
private:
    void cut(uint64_t rows, uint32_t total) {                       // keep `rows` rows and their `total` values; no row: no column
        if (rows == 0) { clear(); return; }
        off_.resize((size_t)rows + 1);
        val_.resize((size_t)total);
    }
    std::vector<uint32_t> off_, val_;
};

// The group slots the grouped search derives from the parents: roots numbered densely — a row's root is its parent, or its own frame
// id where that is WAX_HIP_NO_PARENT. slot_of maps a root to its slot, root_of back, slot(r) is the slot of row r. A root seen keeps
// its slot (so slots are stable under removal), a new one takes the next, and numbering starts over once there are more than
// 2 * count + 16 slots. epoch() moves whenever it starts over: the roots a reader uploaded under an earlier epoch are void.
class GroupSlots {
public:
    uint64_t rows() const { return slot_.size(); }
    uint64_t n_slots() const { return root_.size(); }
    const uint32_t* slots() const { return slot_.data(); }
    const uint64_t* roots() const { return root_.data(); }
    uint64_t epoch() const { return epoch_; }
    // Number rows [from, count); returns the lowest row whose slot may have changed (0 where numbering started over).
    uint64_t number(uint64_t from, uint64_t count, const DenseColumn<uint64_t>& parents, const uint64_t* ids) {
        number_from(from, count, parents, ids);
        if (root_.size() <= 2ull * count + 16ull) return from;
        slot_of_.clear(); root_.clear(); ++epoch_;                  // removals left most slots without a row
        number_from(0, count, parents, ids);
        return 0;
    }
    void clear() { slot_of_.clear(); root_.clear(); slot_.clear(); ++epoch_; }
private:
    void number_from(uint64_t r0, uint64_t count, const DenseColumn<uint64_t>& parents, const uint64_t* ids) {
        slot_.resize((size_t)count);
        for (uint64_t r = r0; r < count; ++r) {
            const uint64_t p = parents.at(r);
            const uint64_t root = p != WAX_HIP_NO_PARENT ? p : ids[(size_t)r];
            auto it = slot_of_.find(root);
            if (it == slot_of_.end()) {
                it = slot_of_.emplace(root, (uint32_t)root_.size()).first;
                root_.push_back(root);
            }
            slot_[(size_t)r] = it->second;
        }
    }
    std::unordered_map<uint64_t, uint32_t> slot_of_;
    std::vector<uint64_t> root_;
    std::vector<uint32_t> slot_;
    uint64_t epoch_ = 0;
};

// The four columns of one store and the marks of their three device copies: the attribute pair (timestamps and flags, always of one
// length), the slot column derived from the parents, the term CSR. One operation per mutation the store knows; each marks from the
// lowest row it moved. A removal behind the attribute columns moves nothing on the device either (those rows are (0, 0) there too) and
// marks nothing; the slot column and the term offsets have an entry for every row of the store, so there every removal marks, while
// their column exists. A column that a mutation leaves empty is a column that never existed: its mark and what is derived from it
// start over.
class RowColumns {
public:
    const DenseColumn<int64_t>& ts() const { return ts_; }
    const DenseColumn<uint32_t>& flags() const { return flags_; }
    const DenseColumn<uint64_t>& parents() const { return parents_; }
    const TermColumn& terms() const { return terms_; }
    const GroupSlots& slots() const { return slots_; }
    bool has_attributes() const { return !ts_.empty(); }
    uint64_t attr_rows() const { return ts_.rows(); }
    UploadMark& attr_mark() { return attr_mark_; }
    UploadMark& group_mark() { return group_mark_; }
    UploadMark& term_mark() { return term_mark_; }

    // ---- the setters (row < count; in call order, so the last entry of a repeated id wins) ----
    void set_attributes(uint64_t row, uint64_t count, const int64_t* ts, const uint32_t* flags) {   // either may be null: left as it is
        ts_.cover(row, count); flags_.cover(row, count);
        if (ts) ts_.set(row, count, *ts);
        if (flags) flags_.set(row, count, *flags);
        attr_mark_.note(row);
    }
    void set_parent(uint64_t row, uint64_t count, uint64_t parent) {
        parents_.set(row, count, parent);
        group_mark_.note(row);
    }
    void commit_terms(const TermPlan& p, const TermRows& rows) {    // TermColumn::commit's conditions
        terms_.commit(p, rows);
        term_mark_.note(rows.front().first);
    }
    // ---- the group slots (ensure_groups; not on a store without parents) ----
    bool groups_current(uint64_t count) const { return group_mark_.from(count) == count && slots_.rows() == count; }
    // Number the slots of rows [lowest marked or first appended, count): returns the lowest row whose slot a device copy has yet to
    // receive. The caller uploads from there and settles group_mark().
    uint64_t number_groups(uint64_t count, const uint64_t* ids) { return slots_.number(group_mark_.from(count), count, parents_, ids); }

    // ---- the mutations of the store ----
    // rows rem[0 .. m) (ascending, unique) leave the store
    template <typename Row>
    void remove_rows(const Row* rem, size_t m) {
        if (m == 0) return;
        const uint64_t lowest = rem[0];
        if (lowest < ts_.rows()) {
            ts_.erase_rows(rem, m); flags_.erase_rows(rem, m);
            moved(ts_.empty(), attr_mark_, lowest);
        }
        if (!parents_.empty()) {
            parents_.erase_rows(rem, m);
            if (parents_.empty()) slots_.clear();                   // every row left is its own root
            moved(parents_.empty(), group_mark_, lowest);
        }
        if (!terms_.empty()) {
            terms_.erase_rows(rem, m);
            moved(terms_.empty(), term_mark_, lowest);
        }
    }
    void remove_row(uint64_t row) { remove_rows(&row, 1); }
    // May this store take every row of `src`? (asked before any row moves; changes nothing)
    bool can_take(const RowColumns& src) const { return terms_.can_append(src.terms_); }
    // Every row of `src` has become rows dst_before .. of this store (can_take(src) held); src is left without columns.
    void take_all(RowColumns& src, uint64_t dst_before) {
        if (!src.ts_.empty()) {
            ts_.append(src.ts_, dst_before); flags_.append(src.flags_, dst_before);
            attr_mark_.note(dst_before);
        }
        if (!src.parents_.empty()) {
            parents_.append(src.parents_, dst_before);
            group_mark_.note(dst_before);
        }
        if (!src.terms_.empty()) {
            terms_.append(src.terms_, dst_before);
            term_mark_.note(dst_before);
        }
        src.clear();
    }
    // The store is back at `rows` rows (a move that failed half way took its appended rows back).
    void truncate(uint64_t rows) {
        ts_.truncate(rows); flags_.truncate(rows); parents_.truncate(rows); terms_.truncate(rows);
        if (parents_.empty()) slots_.clear();
        moved(ts_.empty(), attr_mark_, rows);
        moved(parents_.empty(), group_mark_, rows);
        moved(terms_.empty(), term_mark_, rows);
    }
    // Every row holds the defaults again (deserialize: MV2V has no field for any column; a shard that was emptied).
    void clear() {
        ts_.clear(); flags_.clear(); parents_.clear(); terms_.clear(); slots_.clear();
        attr_mark_.reset(); group_mark_.reset(); term_mark_.reset();
    }
private:
    static void moved(bool emptied, UploadMark& mark, uint64_t row) {
        if (emptied) mark.reset(); else mark.note(row);
    }
    DenseColumn<int64_t> ts_{0};
    DenseColumn<uint32_t> flags_{0u};
    DenseColumn<uint64_t> parents_{WAX_HIP_NO_PARENT};
    TermColumn terms_;
    GroupSlots slots_;
    UploadMark attr_mark_, group_mark_, term_mark_;
};
