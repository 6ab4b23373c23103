// derived_rows.h — how far the three structures derived from the store's rows and ids have followed it: the bf16 mirror, the 8-bit
// code mirror and the id -> row table. Plain C++17 over the standard library: no HIP, no device pointer, no mutex, so
// tests/derived_rows/driver.cpp holds it to a naive model on the CPU. The engine (engine_types.inc) keeps one DerivedRows and, in
// BatchMirror and IdHash, only what is on the device or about it: pointers, capacities, build mutexes, ready events, counters.
//
// Each structure is a RowFill: rows [0, rows) match the store unless a restart is pending. What a mutation of the store does to each:
//
//   DerivedRows::              bf16 mirror (DirtyRowFill)                          code mirror          id -> row table
//   appended()                 not current: [rows, count) to convert               not current          not current
//   overwritten(row)           a held row is listed (past the cap: restart);       restart              — (the id keeps its row)
//                              a row at or behind the fill goes with the appended
//   removed(rem, m, followed)  holds rem[0] and followed: the fill drops by the    restart              restart (every later row
//   removed(row, followed)     removed rows below it, the listed rows are                               changed its number)
//                              renumbered or dropped; held and not followed:
//                              restart; not held: not current
//   replaced()                 restart                                             restart              restart
//   lost()                     restart                                             restart              — (a device pass over the
//                                                                                                         mirrors failed, no row moved)
//
// Every one of them also ends the run of requests that wanted() counts, for both mirrors. Writers hold the exclusive engine lock. A reader
// (ensure_mirror, ensure_mirror8, ensure_idhash) holds its structure's build mutex under the shared lock: begin(count), build rows
// [from, count) — from zeroed scalar words where `scratch` —, take_dirty() and convert those, settle(count). A reader whose buffers had
// to be allocated anew without their contents, or whose build may have left them in doubt, calls restart() itself: that is no mutation
// and leaves the run of requests alone. current(), restarting(), rows() and pending() may be read without the mutex: planning figures,
// racy but defined.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <vector>

constexpr size_t kMirrorMaxDirty = 4096;   // overwritten rows remembered one by one; beyond that the bf16 mirror is converted again as a whole

class RowFill {
public:
    struct Build {
        uint64_t from;    // the first row to build
        bool scratch;     // the structure starts over: its scalar words (running maxima, the table's slots) are zeroed first
    };
    // ---- writers (DerivedRows), and restart() for a reader as well ----
    void appended() { current_ = false; }
    void restart() { current_ = false; restarting_ = true; }
    // ---- the reader, under the structure's build mutex ----
    Build begin(uint64_t count) {
        const bool scratch = restarting_;
        if (scratch) { rows_ = 0; restarting_ = false; }
        if (rows_ > count) rows_ = count;             // (cannot happen: a removal lowers the fill or restarts it)
        return Build{rows_, scratch};
    }
    void settle(uint64_t count) { rows_ = count; current_.store(true, std::memory_order_release); }
    // ---- lock-free ----
    bool current() const { return current_.load(std::memory_order_acquire); }    // the fast path: rows == count, nothing listed, no restart pending
    bool restarting() const { return restarting_; }
    uint64_t rows() const { return rows_; }
    bool wanted() { return wanted_.fetch_add(1) >= 2; }   // true from the third request in a row since the last mutation on
    void mutated() { wanted_ = 0; }                       // (DerivedRows: every mutation of the store ends the run)
protected:
    std::atomic<uint64_t> rows_{0};
private:
    std::atomic<bool> current_{false};
    std::atomic<bool> restarting_{true};
    std::atomic<int> wanted_{0};
};

// A RowFill that remembers up to `cap` overwritten rows below the fill one by one, and follows removals.
class DirtyRowFill : public RowFill {
public:
    explicit DirtyRowFill(size_t cap = kMirrorMaxDirty) : cap_(cap) {}
    bool holds(uint64_t row) const { return !restarting() && row < rows(); }
    void overwritten(uint64_t row) {
        appended();
        if (!holds(row)) return;                          // not converted yet: it goes with the appended range, or with everything
        if (dirty_.size() >= cap_) { restart(); return; }
        dirty_.push_back((uint32_t)row);
        n_dirty_ = dirty_.size();
    }
    // rows rem[0 .. m) (ascending, distinct, m >= 1) left the store and, where the fill holds rem[0], the structure's rows with them
    void removed(const uint32_t* rem, size_t m) {
        appended();
        if (!holds(rem[0])) return;
        auto rank = [&](uint64_t r) { return (uint64_t)(std::lower_bound(rem, rem + m, (uint32_t)std::min<uint64_t>(r, 0xffffffffull)) - rem); };
        rows_ -= rank(rows_);
        size_t w = 0;
        for (const uint32_t r : dirty_)
            if (!std::binary_search(rem, rem + m, r)) dirty_[w++] = r - (uint32_t)rank(r);
        dirty_.resize(w);
        n_dirty_ = w;
    }
    Build begin(uint64_t count) {
        const Build b = RowFill::begin(count);
        if (b.scratch) { dirty_.clear(); n_dirty_ = 0; }
        return b;
    }
    // the listed rows, ascending and distinct, for the reader to convert; the list is empty afterwards
    std::vector<uint32_t> take_dirty() {
        std::vector<uint32_t> out;
        out.swap(dirty_);
        n_dirty_ = 0;
        std::sort(out.begin(), out.end());
        out.erase(std::unique(out.begin(), out.end()), out.end());
        return out;
    }
    // rows the next reader would convert (an overwritten row counts once per overwrite)
    uint64_t pending(uint64_t count) const {
        if (restarting()) return count;
        const uint64_t rows = this->rows();
        return (count > rows ? count - rows : 0) + n_dirty_.load();
    }
private:
    const size_t cap_;
    std::vector<uint32_t> dirty_;          // rows below the fill overwritten since their conversion
    std::atomic<uint64_t> n_dirty_{0};     // dirty_.size(), kept beside it for pending()
};

// The three fills of one store: one operation per mutation (the table at the top).
struct DerivedRows {
    DirtyRowFill bf16;
    RowFill codes, idtable;
    explicit DerivedRows(size_t dirty_cap = kMirrorMaxDirty) : bf16(dirty_cap) {}
    void appended() { mutated(); bf16.appended(); codes.appended(); idtable.appended(); }
    void overwritten(uint64_t row) { mutated(); bf16.overwritten(row); codes.restart(); }
    // `followed`: the bf16 mirror's rows moved on the device as the store's did (asked only where it holds rem[0])
    void removed(const uint32_t* rem, size_t m, bool followed) {
        mutated();
        if (followed || !bf16.holds(rem[0])) bf16.removed(rem, m); else bf16.restart();
        codes.restart(); idtable.restart();
    }
    void removed(uint64_t row, bool followed) { const uint32_t r = (uint32_t)row; removed(&r, 1, followed); }
    void replaced() { mutated(); bf16.restart(); codes.restart(); idtable.restart(); }
    void lost() { mutated(); bf16.restart(); codes.restart(); }
private:
    void mutated() { bf16.mutated(); codes.mutated(); }
};
