// tests/row_columns/driver.cpp — wax_amd/csrc/row_columns.h against a naive model, on the CPU (tests/test_row_columns_cpu.py compiles
// this with -fsanitize=address,undefined and runs it; no GPU, no engine).
//
// Seeded random sequences of every mutation the store knows run on two small stores (at most kMaxRows rows, so that every edge occurs
// often). The model is one full-length record per row, no shortcuts. After every operation every row of every column must read as the
// model's, rows behind the column included. The point of the test is the DEVICE SHADOW: beside each column, and beside the slot
// column and the root table, the driver keeps a copy that only "a reader arrives" touches, and a reader copies only the rows
// [from(count), count) that the column's mark asks for, as ensure_attrs / ensure_groups / ensure_terms do. A mutation that forgets to
// lower a mark leaves the shadow wrong. The driver counts the states it entered and fails if one of kStates is missing.
//
// usage: driver [sequences [operations per sequence [first seed]]]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "row_columns.h"

namespace {

constexpr uint64_t kMaxRows = 64;
constexpr uint32_t kGarbage = 0xdeadbeefu;      // what freshly allocated "device" memory holds

const char* const kStates[] = {
    // the host-side entries of COLUMN_CLASSES (tests/store_sequence_ref.py), per column where a column can enter them
    "attrs_first_set", "attrs_set_behind_column", "parents_first_set", "parents_set_behind_column", "terms_first_set", "terms_set_behind_column",
    "attrs_remove_below_column", "attrs_remove_behind_column", "attrs_remove_batch_straddles_column_end",
    "parents_remove_below_column", "parents_remove_behind_column", "parents_remove_batch_straddles_column_end",
    "terms_remove_below_column", "terms_remove_behind_column", "terms_remove_batch_straddles_column_end",
    "attrs_emptied", "parents_emptied", "terms_emptied",
    "terms_same_size_overwrite", "terms_resize_rebuild", "terms_all_sets_empty", "parents_renumber_from_scratch", "three_columns_different_lengths",
    // the moves between two stores
    "move_into_store_without_columns", "move_into_columns_ending_below_dst_before", "move_from_store_without_columns", "truncate_after_partial_move",
    "move_onto_rows_a_device_copy_holds",
    // what the readers must have met for the shadow check to mean something
    "reader_growth_keeps_prefix", "reader_uploads_suffix_only", "reader_finds_column_current", "reader_roots_sent_again",
};

std::map<std::string, uint64_t> g_entered;
uint64_t g_seed = 0, g_op = 0;
const char* g_what = "";

void enter(const std::string& s) { g_entered[s] += 1; }

[[noreturn]] void die(const std::string& msg) {
    std::printf("FAILED seed %llu op %llu (%s): %s\n", (unsigned long long)g_seed, (unsigned long long)g_op, g_what, msg.c_str());
    std::exit(1);
}
#define CHECK(cond, msg) do { if (!(cond)) die(std::string(#cond) + " — " + (msg)); } while (0)

struct ModelRow {
    uint64_t id = 0;
    int64_t ts = 0;
    uint32_t flags = 0;
    uint64_t parent = WAX_HIP_NO_PARENT;
    std::vector<uint32_t> terms;                 // ascending, distinct
    uint64_t root() const { return parent != WAX_HIP_NO_PARENT ? parent : id; }
};

struct Store {
    std::vector<ModelRow> m;                     // the model
    RowColumns cols;                             // the code under test
    // the device shadow: what the last readers left
    std::vector<int64_t> d_ts;
    std::vector<uint32_t> d_flags, d_slot, d_off, d_val;
    std::vector<uint64_t> d_root;
    uint64_t root_dev = 0, root_epoch = 0;
    uint64_t count() const { return m.size(); }
    std::vector<uint64_t> ids() const {
        std::vector<uint64_t> v;
        for (const ModelRow& r : m) v.push_back(r.id);
        return v;
    }
};

struct Rng {
    std::mt19937_64 g;
    explicit Rng(uint64_t seed) : g(seed) {}
    uint64_t below(uint64_t n) { return n == 0 ? 0 : g() % n; }
    bool one_in(uint64_t n) { return below(n) == 0; }
};

// ---- the checks after every operation -------------------------------------------------------------------------------------------

void check_slots(const Store& s) {
    const GroupSlots& g = s.cols.slots();
    CHECK(g.rows() == s.count(), "a current slot column has one entry per row");
    std::map<uint32_t, uint64_t> root_of_slot;
    std::map<uint64_t, uint32_t> slot_of_root;
    for (uint64_t r = 0; r < s.count(); ++r) {
        const uint32_t slot = g.slots()[r];
        CHECK(slot < g.n_slots(), "slot inside the root table");
        CHECK(g.roots()[slot] == s.m[r].root(), "slot_root[slot[r]] is row r's root");
        CHECK(root_of_slot.emplace(slot, s.m[r].root()).first->second == s.m[r].root(), "rows of one slot share a root");
        CHECK(slot_of_root.emplace(s.m[r].root(), slot).first->second == slot, "rows of one root share a slot");
    }
}

void check_store(const Store& s) {
    const RowColumns& c = s.cols;
    const uint64_t count = s.count();
    CHECK(c.ts().rows() == c.flags().rows() && c.attr_rows() == c.ts().rows(), "timestamps and flags are of one length");
    CHECK(c.attr_rows() <= count && c.parents().rows() <= count && c.terms().rows() <= count, "no column is longer than the store");
    CHECK(c.has_attributes() == (c.attr_rows() != 0), "has_attributes");
    CHECK(c.terms().empty() == (c.terms().rows() == 0), "a term column that covers no row is no column");
    if (c.parents().empty()) CHECK(c.slots().rows() == 0 && c.slots().n_slots() == 0, "no slots on a store without parents");
    uint64_t sum = 0;
    for (uint64_t r = 0; r < count + 3; ++r) {                      // (three rows behind the store as well: the defaults)
        const ModelRow dflt;
        const ModelRow& want = r < count ? s.m[r] : dflt;
        CHECK(c.ts().at(r) == want.ts, "timestamp of row " + std::to_string(r));
        CHECK(c.flags().at(r) == want.flags, "flags of row " + std::to_string(r));
        CHECK(c.parents().at(r) == want.parent, "parent of row " + std::to_string(r));
        const TermColumn::Span sp = c.terms().span(r);
        CHECK(sp.size() == want.terms.size() && std::equal(sp.begin, sp.end, want.terms.begin()), "term set of row " + std::to_string(r));
        sum += want.terms.size();
    }
    CHECK(c.terms().total() == sum, "the total is the model's sum");
    if (!c.terms().empty()) {
        CHECK(c.terms().offset(0) == 0, "first offset");
        for (uint64_t r = 0; r < c.terms().rows(); ++r) CHECK(c.terms().offset(r) <= c.terms().offset(r + 1), "offsets never decrease");
        CHECK(c.terms().offset(c.terms().rows()) == c.terms().total() && c.terms().offset(count + 5) == c.terms().total(), "the last offset is the number of values");
    }
    // a slot column that calls itself current is current: a mutation that did not lower the group mark fails here
    if (!c.parents().empty() && c.groups_current(count)) check_slots(s);
    const uint64_t la = c.attr_rows(), lp = c.parents().rows(), lt = c.terms().rows();
    if (la && lp && lt && la != lp && lp != lt && la != lt && std::max(la, std::max(lp, lt)) < count) enter("three_columns_different_lengths");
}

// ---- the readers: what ensure_attrs / ensure_groups / ensure_terms do, with vectors for device memory ---------------------------

template <typename T>
void grow_keeping(std::vector<T>& dev, uint64_t cap, uint64_t keep) {
    std::vector<T> fresh((size_t)cap, (T)kGarbage);
    std::copy(dev.begin(), dev.begin() + (ptrdiff_t)keep, fresh.begin());
    dev.swap(fresh);
}

void read_attrs(Store& s, Rng& rng) {
    RowColumns& c = s.cols;
    const uint64_t count = s.count(), na = c.attr_rows();
    if (na == 0) return;                                            // the kernel reads every row as (0, 0): nothing is allocated
    UploadMark& mark = c.attr_mark();
    if (s.d_ts.size() < count) {
        const uint64_t keep = mark.from(s.d_ts.size());
        if (keep > 0) enter("reader_growth_keeps_prefix");
        const uint64_t cap = count + rng.below(8);
        grow_keeping(s.d_ts, cap, keep); grow_keeping(s.d_flags, cap, keep);
        mark.note(keep);
    }
    const uint64_t from = mark.from(count);
    if (from == count) enter("reader_finds_column_current");
    else if (from > 0) enter("reader_uploads_suffix_only");
    const uint64_t host_end = std::min(na, count);
    for (uint64_t r = from; r < count; ++r) {
        s.d_ts[r] = r < host_end ? c.ts().data()[r] : 0;
        s.d_flags[r] = r < host_end ? c.flags().data()[r] : 0u;
    }
    mark.settle(count);
    for (uint64_t r = 0; r < count; ++r)
        CHECK(s.d_ts[r] == s.m[r].ts && s.d_flags[r] == s.m[r].flags, "attribute shadow of row " + std::to_string(r));
}

void read_groups(Store& s, Rng& rng) {
    RowColumns& c = s.cols;
    const uint64_t count = s.count();
    if (c.parents().empty()) return;                                // slot = row, the roots are the frame ids
    if (!c.groups_current(count)) {
        const uint64_t epoch_before = c.slots().epoch();
        const std::vector<uint64_t> ids = s.ids();
        uint64_t from = c.number_groups(count, ids.data());
        if (c.slots().epoch() != epoch_before) { enter("parents_renumber_from_scratch"); CHECK(from == 0, "numbering from scratch moves every slot"); }
        if (s.root_epoch != c.slots().epoch()) {
            if (s.root_dev > 0) enter("reader_roots_sent_again");
            s.root_epoch = c.slots().epoch();
            s.root_dev = 0;
        }
        const uint64_t n_roots = c.slots().n_slots();
        CHECK(n_roots <= 2 * count + 16, "numbering starts over above 2 * count + 16 slots");
        if (s.d_slot.size() < count) { s.d_slot.assign((size_t)(count + rng.below(8)), kGarbage); from = 0; }      // sent again whole
        if (s.d_root.size() < n_roots) { s.d_root.assign((size_t)(n_roots + rng.below(8)), kGarbage); s.root_dev = 0; }
        if (from > 0 && from < count) enter("reader_uploads_suffix_only");
        CHECK(s.root_dev <= n_roots, "roots uploaded under this numbering");
        std::copy(c.slots().slots() + from, c.slots().slots() + count, s.d_slot.begin() + (ptrdiff_t)from);
        std::copy(c.slots().roots() + s.root_dev, c.slots().roots() + n_roots, s.d_root.begin() + (ptrdiff_t)s.root_dev);
        s.root_dev = n_roots;
    } else {
        enter("reader_finds_column_current");
    }
    c.group_mark().settle(count);
    check_slots(s);
    for (uint64_t r = 0; r < count; ++r) CHECK(s.d_slot[r] == c.slots().slots()[r], "slot shadow of row " + std::to_string(r));
    for (uint64_t i = 0; i < c.slots().n_slots(); ++i) CHECK(s.d_root[i] == c.slots().roots()[i], "root shadow of slot " + std::to_string(i));
}

void read_terms(Store& s, Rng& rng) {
    RowColumns& c = s.cols;
    const TermColumn& terms = c.terms();
    if (terms.empty()) return;                                      // decided on the host: nothing is touched
    UploadMark& mark = c.term_mark();
    const uint64_t count = s.count(), total = terms.total();
    uint64_t from = mark.from(count);
    bool current = mark.current(count);
    if (s.d_off.size() < count + 1 || s.d_val.size() < total) {
        const uint64_t keep = s.d_off.empty() ? 0 : std::min<uint64_t>(from, s.d_off.size() - 1);
        const uint64_t keep_val = std::min<uint64_t>(terms.offset(keep), s.d_val.size());
        if (keep > 0) enter("reader_growth_keeps_prefix");
        grow_keeping(s.d_off, std::max<uint64_t>(s.d_off.size(), count + 1 + rng.below(8)), keep);
        grow_keeping(s.d_val, std::max<uint64_t>(s.d_val.size(), total + rng.below(16)), keep > 0 ? keep_val : 0);
        mark.note(keep);
        from = mark.from(count);
        current = false;
    }
    if (!current) {
        if (from > 0 && from < count) enter("reader_uploads_suffix_only");
        for (uint64_t r = from; r <= count; ++r) s.d_off[r] = terms.offset(r);
        const uint32_t v0 = terms.offset(from);
        std::copy(terms.values() + v0, terms.values() + total, s.d_val.begin() + v0);
    } else {
        enter("reader_finds_column_current");
    }
    mark.settle(count);
    uint64_t at = 0;
    for (uint64_t r = 0; r < count; ++r) {
        CHECK(s.d_off[r] == at, "offset shadow of row " + std::to_string(r));
        for (uint32_t t : s.m[r].terms) CHECK(s.d_val[at++] == t, "value shadow of row " + std::to_string(r));
    }
    CHECK(s.d_off[count] == at && at == total, "offset shadow behind the last row");
}

// ---- the mutations ----------------------------------------------------------------------------------------------------------------

uint64_t g_next_id = 1, g_next_root = 1ull << 40;

void op_append(Store& s, Rng& rng) {
    // appends fill a store to half of kMaxRows, so that two stores usually fit into one: only a move makes a larger one
    const uint64_t room = s.count() < kMaxRows / 2 ? kMaxRows / 2 - s.count() : 0;
    for (uint64_t i = 0, k = 1 + rng.below(std::min<uint64_t>(room, 6)); i < k && room; ++i) { ModelRow r; r.id = g_next_id++; s.m.push_back(r); }
}

// a row for a setter: now and then one at or behind the column's end
uint64_t pick_row(const Store& s, uint64_t column_rows, Rng& rng) {
    if (column_rows < s.count() && rng.one_in(3)) return column_rows + rng.below(s.count() - column_rows);
    return rng.below(s.count());
}

void op_set_attributes(Store& s, Rng& rng) {
    if (s.count() == 0) return;
    const uint64_t mode = rng.below(4);                             // both, timestamps only, flags only, both
    for (uint64_t i = 0, n = 1 + rng.below(5); i < n; ++i) {
        const uint64_t row = i > 0 && rng.one_in(4) ? rng.below(s.count()) : pick_row(s, s.cols.attr_rows(), rng);
        const int64_t ts = (int64_t)rng.below(1000000) - 500000;
        const uint32_t fl = (uint32_t)rng.below(1u << 20);
        if (s.cols.attr_rows() == 0) enter("attrs_first_set");
        else if (row >= s.cols.attr_rows()) enter("attrs_set_behind_column");
        s.cols.set_attributes(row, s.count(), mode != 2 ? &ts : nullptr, mode != 1 ? &fl : nullptr);
        if (mode != 2) s.m[row].ts = ts;
        if (mode != 1) s.m[row].flags = fl;
    }
}

void op_set_parents(Store& s, Rng& rng) {
    if (s.count() == 0) return;
    uint64_t shared_root = g_next_root++;
    for (uint64_t i = 0, n = 1 + rng.below(6); i < n; ++i) {
        const uint64_t row = pick_row(s, s.cols.parents().rows(), rng);
        uint64_t parent = WAX_HIP_NO_PARENT;
        switch (rng.below(5)) {
            case 0: break;
            case 1: parent = s.m[rng.below(s.count())].id; break;   // a held frame
            case 2: parent = shared_root; break;                    // one root for several rows of this call
            default: parent = g_next_root++; break;                 // a root never seen: the slots pile up until numbering starts over
        }
        if (s.cols.parents().empty()) enter("parents_first_set");
        else if (row >= s.cols.parents().rows()) enter("parents_set_behind_column");
        s.cols.set_parent(row, s.count(), parent);
        s.m[row].parent = parent;
    }
}

void op_set_terms(Store& s, Rng& rng) {
    if (s.count() == 0) return;
    const uint64_t mode = rng.below(4);                             // 0: the sizes the rows have, 1: all empty, else: any size
    TermPlan plan;
    TermRows rows;
    plan.e_off.push_back(0);
    std::map<uint64_t, std::vector<uint32_t>> last;                 // in call order the last entry of a repeated row wins
    for (uint64_t i = 0, n = 1 + rng.below(5); i < n; ++i) {
        const uint64_t row = mode == 0 ? rng.below(s.count()) : pick_row(s, s.cols.terms().rows(), rng);
        const uint64_t size = mode == 0 ? s.m[row].terms.size() : mode == 1 ? 0 : rng.below(rng.one_in(8) ? WAX_HIP_TERMS_MAX_PER_ROW + 1 : 5);
        std::set<uint32_t> set;
        while (set.size() < size) set.insert((uint32_t)rng.below(1000));
        plan.flat.insert(plan.flat.end(), set.begin(), set.end());
        plan.e_off.push_back(plan.flat.size());
        rows.emplace_back(row, i);
        last[row].assign(set.begin(), set.end());
    }
    finish_term_rows(&rows);
    CHECK(rows.size() == last.size(), "one entry per row");
    const uint64_t old_rows = s.cols.terms().rows();
    bool resized = false;
    for (const auto& re : rows) resized |= !(re.first < old_rows && plan.len(re.second) == s.m[re.first].terms.size());
    for (const auto& kv : last) s.m[kv.first].terms = kv.second;
    uint64_t sum = 0;
    for (const ModelRow& r : s.m) sum += r.terms.size();
    CHECK(s.cols.terms().total_after(plan, rows) == sum, "the planned total is the model's sum");
    if (s.cols.terms().empty()) enter("terms_first_set");
    else if (rows.back().first >= old_rows) enter("terms_set_behind_column");
    enter(resized ? "terms_resize_rebuild" : "terms_same_size_overwrite");
    s.cols.commit_terms(plan, rows);
    if (sum == 0) enter("terms_all_sets_empty");
}

void note_removal(const char* column, uint64_t column_rows, const std::vector<uint32_t>& rem) {
    if (column_rows == 0) return;
    const bool below = rem.front() < column_rows, behind = rem.back() >= column_rows;
    if (below) enter(std::string(column) + "_remove_below_column");
    if (behind) enter(std::string(column) + "_remove_behind_column");
    if (below && behind) enter(std::string(column) + "_remove_batch_straddles_column_end");
}

void remove_rows(Store& s, const std::vector<uint32_t>& rem, bool one) {
    const uint64_t la = s.cols.attr_rows(), lp = s.cols.parents().rows(), lt = s.cols.terms().rows();
    note_removal("attrs", la, rem); note_removal("parents", lp, rem); note_removal("terms", lt, rem);
    if (one) s.cols.remove_row(rem[0]); else s.cols.remove_rows(rem.data(), rem.size());
    for (size_t i = rem.size(); i-- > 0;) s.m.erase(s.m.begin() + rem[i]);
    if (la && !s.cols.has_attributes()) enter("attrs_emptied");
    if (lp && s.cols.parents().empty()) enter("parents_emptied");
    if (lt && s.cols.terms().empty()) enter("terms_emptied");
}

void op_remove(Store& s, Rng& rng) {
    if (s.count() == 0) return;
    remove_rows(s, {(uint32_t)rng.below(s.count())}, true);
}

void op_remove_batch(Store& s, Rng& rng) {
    if (s.count() == 0) return;
    std::set<uint32_t> rows;
    const uint64_t mode = rng.below(5);
    if (mode == 0) {                                                // a stretch from the front: every row under the shorter columns
        for (uint64_t r = 0, n = 1 + rng.below(s.count()); r < n; ++r) rows.insert((uint32_t)r);
    } else if (mode == 1) {                                         // the tail: nothing moves
        for (uint64_t r = s.count() - 1 - rng.below(std::min<uint64_t>(s.count(), 4)) + 0; r < s.count(); ++r) rows.insert((uint32_t)r);
    } else if (mode == 2 && s.cols.attr_rows() < s.count()) {      // rows behind the attribute columns only: their mark stays where it is
        for (uint64_t i = 0, n = 1 + rng.below(8); i < n; ++i) rows.insert((uint32_t)(s.cols.attr_rows() + rng.below(s.count() - s.cols.attr_rows())));
    } else {
        for (uint64_t i = 0, n = 1 + rng.below(8); i < n; ++i) rows.insert((uint32_t)rng.below(s.count()));
    }
    remove_rows(s, std::vector<uint32_t>(rows.begin(), rows.end()), false);
}

void op_move(Store& src, Store& dst, Rng& rng) {
    if (src.count() == 0 || src.count() + dst.count() > kMaxRows) return;
    CHECK(dst.cols.can_take(src.cols), "stores of this size never reach 2^32 terms");
    const uint64_t dst_before = dst.count();
    const bool src_has = src.cols.has_attributes() || !src.cols.parents().empty() || !src.cols.terms().empty();
    const bool dst_has = dst.cols.has_attributes() || !dst.cols.parents().empty() || !dst.cols.terms().empty();
    if (rng.one_in(4)) {
        // the move fails after some rows were appended: they are taken back, the source still holds every row
        dst.cols.truncate(dst_before);
        enter("truncate_after_partial_move");
        return;
    }
    if (!dst_has && src_has && dst_before > 0) enter("move_into_store_without_columns");
    if (!src_has && dst_has) enter("move_from_store_without_columns");
    if (src_has && dst_has && std::max(dst.cols.attr_rows(), std::max(dst.cols.parents().rows(), dst.cols.terms().rows())) < dst_before)
        enter("move_into_columns_ending_below_dst_before");
    // removals behind the attribute columns mark nothing, so the device copy may reach past dst_before: only the move's own mark
    // has the moved rows uploaded
    if (src.cols.has_attributes() && dst.cols.has_attributes() && dst.cols.attr_mark().from(dst_before + src.count()) > dst_before)
        enter("move_onto_rows_a_device_copy_holds");
    dst.cols.take_all(src.cols, dst_before);
    dst.m.insert(dst.m.end(), src.m.begin(), src.m.end());
    src.m.clear();
    CHECK(!src.cols.has_attributes() && src.cols.parents().empty() && src.cols.terms().empty(), "the source is left without columns");
}

void op_clear(Store& s) {                                           // deserialize: the rows stay, every column is dropped
    s.cols.clear();
    for (ModelRow& r : s.m) { r.ts = 0; r.flags = 0; r.parent = WAX_HIP_NO_PARENT; r.terms.clear(); }
}

void run_sequence(uint64_t seed, uint64_t n_ops) {
    Rng rng(seed);
    Store st[2];
    g_seed = seed;
    for (g_op = 0; g_op < n_ops; ++g_op) {
        Store& s = st[rng.below(2)];
        Store& other = &s == &st[0] ? st[1] : st[0];
        const uint64_t pick = rng.below(100);
        if (pick < 16) { g_what = "append"; op_append(s, rng); }
        else if (pick < 28) { g_what = "set attributes"; op_set_attributes(s, rng); }
        else if (pick < 40) { g_what = "set parents"; op_set_parents(s, rng); }
        else if (pick < 54) { g_what = "set terms"; op_set_terms(s, rng); }
        else if (pick < 62) { g_what = "remove"; op_remove(s, rng); }
        else if (pick < 69) { g_what = "remove batch"; op_remove_batch(s, rng); }
        else if (pick < 75) { g_what = "move all"; op_move(s, other, rng); }
        else if (pick < 76) { g_what = "clear"; op_clear(s); }
        else if (pick < 78) {
            // the one chain the dice rarely throw: the device copy of the attributes reaches past the rows a removal leaves, then rows move in
            g_what = "attribute reader, removal behind the attribute columns, move all";
            read_attrs(s, rng);
            if (s.cols.has_attributes() && s.cols.attr_rows() < s.count()) remove_rows(s, {(uint32_t)(s.count() - 1)}, true);
            op_move(other, s, rng);
        }
        else {
            g_what = "a reader arrives";
            if (rng.below(3)) read_attrs(s, rng);
            if (rng.below(3)) read_groups(s, rng);
            if (rng.below(3)) read_terms(s, rng);
        }
        check_store(st[0]);
        check_store(st[1]);
    }
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t n_seq = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 40;
    const uint64_t n_ops = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 400;
    const uint64_t seed0 = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 4101;
    for (uint64_t i = 0; i < n_seq; ++i) run_sequence(seed0 + i, n_ops);
    std::vector<std::string> missing;
    for (const char* name : kStates) {
        std::printf("state %s %llu\n", name, (unsigned long long)g_entered[name]);
        if (g_entered[name] == 0) missing.push_back(name);
    }
    for (const auto& kv : g_entered) {
        if (std::find_if(std::begin(kStates), std::end(kStates), [&](const char* n) { return kv.first == n; }) == std::end(kStates)) {
            std::printf("FAILED: state %s is entered but not listed\n", kv.first.c_str());
            return 1;
        }
    }
    if (!missing.empty()) {
        std::printf("FAILED: states never entered:");
        for (const std::string& m : missing) std::printf(" %s", m.c_str());
        std::printf("\n");
        return 1;
    }
    std::printf("ok: %llu sequences of %llu operations, %zu states\n", (unsigned long long)n_seq, (unsigned long long)n_ops, std::size(kStates));
    return 0;
}
