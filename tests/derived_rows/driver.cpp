// tests/derived_rows/driver.cpp — wax_amd/csrc/derived_rows.h against a naive model and three device shadows, on the CPU
// (tests/test_derived_rows_cpu.py compiles this with -fsanitize=address,undefined and runs it; no GPU, no engine).
//
// Seeded random sequences of every mutation the store knows run on a small store (at most kMaxRows rows and a cap of kSmallCap listed
// rows, so that every edge occurs often; one scripted sequence runs the real cap). The store is a vector of rows {id, value}: an id is
// drawn when a row is appended, a value at every write. Two independent things follow it:
//   - the MODEL keeps, per row of the store, whether each structure holds the row and how often it was overwritten since, plus one
//     "everything again" flag per structure. Its figures are recomputed from those arrays: it has no fill, no list and no renumbering;
//   - the SHADOWS stand for device memory: a reader (what ensure_mirror, ensure_mirror8 and ensure_idhash do, with their growth rules)
//     writes only the rows begin() and take_dirty() name, wipes a shadow where begin() says "from scratch", and a removal moves a
//     shadow's rows only where the driver plays one that the mirror followed.
// After every reader its shadow must equal the store on [0, count) and the rows it converted must be the model's prediction: the
// numbers behind mirror_rows_converted, mirror8_conversions / mirror8_rows_converted and idhash_rows_inserted. The driver counts the
// states it entered and fails if one of kStates is missing.
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

#include "derived_rows.h"

namespace {

constexpr uint64_t kMaxRows = 72, kFirstCapacity = 8, kMaxCapacity = 512, kFirstSlots = 16;
constexpr size_t kSmallCap = 8;
constexpr uint64_t kGarbage = 0xdeadbeefdeadbeefull;   // what freshly allocated "device" memory holds
constexpr uint64_t kEmpty = 0;                          // an empty slot of the id table (ids and values start at 1)

const char* const kStates[] = {
    // the mirror's entries of MIRROR_CLASSES (tests/store_sequence_ref.py) and what the header adds to them
    "upsert_converted", "upsert_above_fill", "upsert_while_restarting", "upserts_cap_listed", "upserts_cap_plus_one_restart",
    "real_cap_listed", "real_cap_plus_one_restart",
    "remove_below_fill", "remove_dirty_below", "remove_dirty_above", "remove_dirty_at", "remove_above_fill", "remove_not_followed",
    "remove_batch_straddle", "remove_batch_dirty_removed", "remove_batch_dirty_surviving", "remove_batch_tail_only",
    "remove_batch_not_followed", "remove_batch_above_fill",
    "growth_dirty_pending", "growth_unconverted_pending", "growth_restarts_codes", "growth_restarts_idtable",
    "append_after_settle", "replaced_with_dirty_pending", "lost_then_read",
    "wanted_third_request_builds", "wanted_reset_by_mutation", "reader_finds_everything_current",
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

struct Rng {
    std::mt19937_64 g;
    explicit Rng(uint64_t seed) : g(seed) {}
    uint64_t below(uint64_t n) { return n == 0 ? 0 : g() % n; }
    bool one_in(uint64_t n) { return below(n) == 0; }
};

struct Row { uint64_t id, value; };

// What the model knows of one structure: per store row, does the structure hold it as it is (`hits` overwrites since it last did)?
struct Held { bool held = false; uint32_t hits = 0; };
struct ModelOf {
    std::vector<Held> rows;      // one per store row, in row order
    bool all = true;             // everything again, whatever `rows` says
    bool built = false;          // a reader has been here
    uint64_t cap = 0;            // rows (slots, for the table) its device memory has room for
    uint64_t requests = 0;       // requests since the last mutation that found it unusable
    bool holds(uint64_t r) const { return !all && r < rows.size() && rows[r].held; }
    uint64_t hits() const { uint64_t n = 0; for (const Held& h : rows) n += h.held ? h.hits : 0; return n; }
    uint64_t to_convert() const {                                   // distinct rows the next reader converts
        if (all) return rows.size();
        return (uint64_t)std::count_if(rows.begin(), rows.end(), [](const Held& h) { return !h.held || h.hits > 0; });
    }
    void converted() { for (Held& h : rows) h = Held{true, 0}; all = false; built = true; }
    bool wanted() { return requests++ >= 2; }
};

struct Sim {
    explicit Sim(size_t cap) : d(cap), dirty_cap(cap) {}
    std::vector<Row> store;
    uint64_t capacity = kFirstCapacity, next = 1;
    DerivedRows d;                                                  // the code under test
    const size_t dirty_cap;
    ModelOf m, c, h;                                                // bf16 mirror, code mirror, id table
    std::vector<uint64_t> s_m, s_c, s_h;                            // the shadows: values, values, the table's ids by row
    uint64_t max_m = 0, max_c = 0;                                  // the scalar words: a running maximum each
    bool just_lost = false;
    uint64_t count() const { return store.size(); }
    uint64_t fresh() { return next++; }
};

void grow_store(Sim& s, uint64_t required) { while (required > s.capacity) s.capacity *= 2; }

void mutation(Sim& s) {                                             // every mutation ends the runs of requests
    if ((s.m.requests > 0 && s.m.requests < 3) || (s.c.requests > 0 && s.c.requests < 3)) enter("wanted_reset_by_mutation");
    s.m.requests = s.c.requests = 0;
    s.just_lost = false;
}

// ---- the readers ---------------------------------------------------------------------------------------------------------------

void check_shadow(const Sim& s, const std::vector<uint64_t>& shadow, bool ids, const char* what) {
    for (uint64_t r = 0; r < s.count(); ++r)
        CHECK(shadow[r] == (ids ? s.store[r].id : s.store[r].value), std::string(what) + " shadow of row " + std::to_string(r));
}

void read_bf16(Sim& s) {
    DirtyRowFill& f = s.d.bf16;
    const uint64_t count = s.count();
    // the model first: the growth rule (the converted prefix moves over), then the rows to convert
    if (s.m.cap < s.capacity) {
        const bool keeps = !s.m.all && std::any_of(s.m.rows.begin(), s.m.rows.end(), [](const Held& x) { return x.held; });
        if (keeps && s.m.hits() > 0) enter("growth_dirty_pending");
        if (keeps && std::any_of(s.m.rows.begin(), s.m.rows.end(), [](const Held& x) { return !x.held; })) enter("growth_unconverted_pending");
        if (!keeps) s.m.all = true;
        s.m.cap = s.capacity;
    }
    const uint64_t predicted = s.m.to_convert();
    if (s.just_lost) enter("lost_then_read");
    const uint64_t not_held = (uint64_t)std::count_if(s.m.rows.begin(), s.m.rows.end(), [](const Held& x) { return !x.held; });
    CHECK(f.pending(count) == (s.m.all ? count : not_held + s.m.hits()), "pending() is the rows not held and one per overwrite");
    s.just_lost = false;
    s.m.converted();
    // ensure_mirror
    uint64_t converted = 0;
    if (!(f.current() && s.s_m.size() >= s.capacity)) {
        if (s.s_m.size() < s.capacity) {
            std::vector<uint64_t> fresh((size_t)s.capacity, kGarbage);
            const uint64_t kept = f.restarting() ? 0 : f.rows();
            if (kept > 0 && !s.s_m.empty()) std::copy(s.s_m.begin(), s.s_m.begin() + (ptrdiff_t)kept, fresh.begin());
            else f.restart();
            s.s_m.swap(fresh);
        }
        const RowFill::Build b = f.begin(count);
        if (b.scratch) { std::fill(s.s_m.begin(), s.s_m.end(), kGarbage); s.max_m = 0; }
        for (uint64_t r = b.from; r < count; ++r) { s.s_m[r] = s.store[r].value; s.max_m = std::max(s.max_m, s.store[r].value); }
        const std::vector<uint32_t> dirty = f.take_dirty();
        CHECK(dirty.size() <= s.dirty_cap, "the list fits the device buffer");
        for (size_t i = 0; i < dirty.size(); ++i) {
            CHECK(dirty[i] < b.from && (i == 0 || dirty[i - 1] < dirty[i]), "listed rows: ascending, distinct, below the fill");
            s.s_m[dirty[i]] = s.store[dirty[i]].value;
            s.max_m = std::max(s.max_m, s.store[dirty[i]].value);
        }
        converted = (count - b.from) + dirty.size();
        f.settle(count);
    }
    CHECK(converted == predicted, "bf16 rows converted: " + std::to_string(converted) + ", the model says " + std::to_string(predicted));
    check_shadow(s, s.s_m, false, "bf16");
    for (const Row& r : s.store) CHECK(s.max_m >= r.value, "the running maximum bounds every row");
    CHECK(f.current() && f.rows() == count && f.pending(count) == 0, "a settled fill");
}

void read_codes(Sim& s) {
    RowFill& f = s.d.codes;
    const uint64_t count = s.count();
    if (s.c.cap < s.capacity) {                                     // the growth rule: the codes do not move over
        if (s.c.holds(0)) enter("growth_restarts_codes");
        s.c.all = true;
        s.c.cap = s.capacity;
    }
    const uint64_t predicted = s.c.to_convert();
    s.c.converted();
    uint64_t converted = 0;
    if (!(f.current() && s.s_c.size() >= s.capacity)) {
        if (s.s_c.size() < s.capacity) { s.s_c.assign((size_t)s.capacity, kGarbage); f.restart(); }
        const RowFill::Build b = f.begin(count);
        if (b.scratch) { std::fill(s.s_c.begin(), s.s_c.end(), kGarbage); s.max_c = 0; }
        for (uint64_t r = b.from; r < count; ++r) { s.s_c[r] = s.store[r].value; s.max_c = std::max(s.max_c, s.store[r].value); }
        converted = count - b.from;
        f.settle(count);
    }
    CHECK(converted == predicted, "code rows converted: " + std::to_string(converted) + ", the model says " + std::to_string(predicted));
    check_shadow(s, s.s_c, false, "code");
    for (const Row& r : s.store) CHECK(s.max_c >= r.value, "the running maximum bounds every row");
    CHECK(f.current() && f.rows() == count, "a settled fill");
}

void read_idtable(Sim& s) {
    RowFill& f = s.d.idtable;
    const uint64_t count = s.count();
    uint64_t want = kFirstSlots;
    while (want < 2 * count) want *= 2;
    if (s.h.cap < want) {                                           // the growth rule: a table that must grow is rebuilt from row 0
        if (s.h.holds(0)) enter("growth_restarts_idtable");
        s.h.all = true;
        s.h.cap = 2 * want;
    }
    const uint64_t predicted = s.h.to_convert();
    s.h.converted();
    uint64_t inserted = 0;
    if (!f.current()) {
        if (s.s_h.size() < want) { s.s_h.assign((size_t)(2 * want), kGarbage); f.restart(); }
        const uint64_t from = f.begin(count).from;
        if (from == 0) std::fill(s.s_h.begin(), s.s_h.end(), kEmpty);   // (the build kernel clears the table in front of row 0)
        for (uint64_t r = from; r < count; ++r) s.s_h[r] = s.store[r].id;
        inserted = count - from;
        f.settle(count);
    }
    CHECK(inserted == predicted, "id table rows inserted: " + std::to_string(inserted) + ", the model says " + std::to_string(predicted));
    check_shadow(s, s.s_h, true, "id table");
    for (uint64_t r = count; r < s.s_h.size(); ++r) CHECK(s.s_h[r] == kEmpty, "no id of a row that left");
}

// A request that would like a mirror: served at once where the mirror is usable as it is (the code mirror also where it only lacks
// appended rows), otherwise by the third such request in a row since the last mutation — mirror8_take, and the small batches of api_batch.inc.
void request(Sim& s, bool codes) {
    ModelOf& mo = codes ? s.c : s.m;
    RowFill& f = codes ? s.d.codes : static_cast<RowFill&>(s.d.bf16);
    const std::vector<uint64_t>& shadow = codes ? s.s_c : s.s_m;
    const bool usable = shadow.size() >= s.capacity && !shadow.empty() && (f.current() || (codes && !f.restarting()));
    if (codes) CHECK(usable == (mo.cap >= s.capacity && mo.cap > 0 && !mo.all), "a code mirror that only lacks appended rows is taken at once");
    if (!usable) {
        const bool third = mo.requests == 2;
        const bool w = f.wanted(), mw = mo.wanted();
        CHECK(w == mw, "wanted() after " + std::to_string(mo.requests - 1) + " requests since the last mutation");
        if (!w) return;
        if (third) enter("wanted_third_request_builds");
    }
    if (codes) read_codes(s); else read_bf16(s);
}

// ---- the mutations ---------------------------------------------------------------------------------------------------------------

void append_row(Sim& s) {
    s.store.push_back(Row{s.fresh(), s.fresh()});
    s.m.rows.push_back(Held{}); s.c.rows.push_back(Held{}); s.h.rows.push_back(Held{});
}

void overwrite_row(Sim& s, uint64_t row) {
    s.store[row].value = s.fresh();
    if (s.m.holds(row)) {
        if (s.m.hits() >= s.dirty_cap) { s.m.all = true; enter(s.dirty_cap == kSmallCap ? "upserts_cap_plus_one_restart" : "real_cap_plus_one_restart"); }
        else {
            s.m.rows[row].hits += 1;
            enter("upsert_converted");
            if (s.m.hits() == s.dirty_cap) enter(s.dirty_cap == kSmallCap ? "upserts_cap_listed" : "real_cap_listed");
        }
    } else if (s.m.built) {
        enter(s.m.all ? "upsert_while_restarting" : "upsert_above_fill");
    }
    s.c.all = true;                                                 // the id keeps its row: the table stays as it is
    s.d.overwritten(row);
    CHECK(s.d.bf16.holds(row) == s.m.holds(row), "holds() after an overwrite");
}

// wax_hip_add_batch: sequential upsert semantics, capacity reserved for "every id new"
void op_add_batch(Sim& s, Rng& rng, bool burst) {
    const uint64_t n = burst ? 6 + rng.below(8) : 1 + rng.below(6);
    mutation(s);
    const bool settled = s.d.bf16.current() && s.d.codes.current() && s.d.idtable.current();
    s.d.appended();
    grow_store(s, s.count() + n);
    for (uint64_t i = 0; i < n; ++i) {
        const bool over = s.count() > 0 && (burst || s.count() >= kMaxRows || rng.one_in(3));
        const uint64_t fill = (uint64_t)std::count_if(s.m.rows.begin(), s.m.rows.end(), [](const Held& x) { return x.held; });
        if (over) overwrite_row(s, burst && s.m.holds(0) && rng.below(8) ? rng.below(fill) : rng.below(s.count()));
        else { append_row(s); if (settled && i == 0) enter("append_after_settle"); }
    }
}

// the mirror's rows below its fill close up as the store's do (mirror_follow_remove, compact_removed_rows); what lies behind them is of no use
void close_up(std::vector<uint64_t>& shadow, const std::vector<uint32_t>& rem, uint64_t fill) {
    std::vector<uint64_t> out;
    for (uint64_t r = 0; r < fill; ++r)
        if (!std::binary_search(rem.begin(), rem.end(), (uint32_t)r)) out.push_back(shadow[r]);
    out.resize(shadow.size(), kGarbage);
    shadow.swap(out);
}

void remove_rows(Sim& s, const std::vector<uint32_t>& rem, bool one, bool device_ok) {
    mutation(s);
    const uint64_t count = s.count(), m = rem.size();
    const bool held = s.m.holds(rem[0]);
    CHECK(s.d.bf16.holds(rem[0]) == held, "holds() in front of a removal");
    const bool moves = rem[0] + m < count;
    const bool followed = held ? (!moves || device_ok) : device_ok;     // (not held: the header does not ask)
    const std::set<uint32_t> gone(rem.begin(), rem.end());
    const std::string p = one ? "remove_" : "remove_batch_";
    if (held && followed) {
        if (one) enter("remove_below_fill");
        else if (!moves) enter("remove_batch_tail_only");
        bool below = false, above = false, at = false, surviving = false;
        for (uint64_t r = 0; r < count; ++r) {
            if (!s.m.rows[r].held || s.m.rows[r].hits == 0) continue;
            below |= r < rem[0]; above |= r > rem[0] && !gone.count((uint32_t)r); at |= gone.count((uint32_t)r) != 0;
            surviving |= r > rem[0] && !gone.count((uint32_t)r);
        }
        if (one) { if (below) enter("remove_dirty_below"); if (above) enter("remove_dirty_above"); if (at) enter("remove_dirty_at"); }
        else {
            if (!s.m.holds(rem.back())) enter("remove_batch_straddle");
            if (at) enter("remove_batch_dirty_removed");
            if (surviving) enter("remove_batch_dirty_surviving");
        }
        if (moves) close_up(s.s_m, rem, s.d.bf16.rows());
    } else if (held) {
        enter(p + "not_followed");
    } else if (s.m.built && !s.m.all) {
        enter(p + "above_fill");
    }
    if (one) s.d.removed((uint64_t)rem[0], followed); else s.d.removed(rem.data(), rem.size(), followed);
    // the model: the rows leave every array; a mirror that held them and could not follow, the code mirror and the table start over
    for (size_t i = rem.size(); i-- > 0;) {
        s.store.erase(s.store.begin() + rem[i]);
        s.m.rows.erase(s.m.rows.begin() + rem[i]); s.c.rows.erase(s.c.rows.begin() + rem[i]); s.h.rows.erase(s.h.rows.begin() + rem[i]);
    }
    if (held && !followed) s.m.all = true;
    s.c.all = s.h.all = true;
}

void op_remove(Sim& s, Rng& rng) {
    if (s.count() == 0) return;
    remove_rows(s, {(uint32_t)rng.below(s.count())}, true, !rng.one_in(6));
}

void op_remove_batch(Sim& s, Rng& rng) {
    if (s.count() == 0) return;
    std::set<uint32_t> rows;
    const uint64_t mode = rng.below(4);
    if (mode == 0) {                                                // the tail: nothing moves
        for (uint64_t r = s.count() - 1 - rng.below(std::min<uint64_t>(s.count(), 4)); r < s.count(); ++r) rows.insert((uint32_t)r);
    } else if (mode == 1 && s.d.bf16.holds(0) && s.d.bf16.rows() < s.count()) {   // across the fill
        rows.insert((uint32_t)rng.below(s.d.bf16.rows()));
        rows.insert((uint32_t)(s.d.bf16.rows() + rng.below(s.count() - s.d.bf16.rows())));
    } else {
        for (uint64_t i = 0, n = 1 + rng.below(8); i < n; ++i) rows.insert((uint32_t)rng.below(s.count()));
    }
    remove_rows(s, std::vector<uint32_t>(rows.begin(), rows.end()), false, !rng.one_in(6));
}

void op_replace(Sim& s, Rng& rng) {                                 // deserialize: every row is new, capacity only grows
    mutation(s);
    if (!s.m.all && s.m.hits() > 0) enter("replaced_with_dirty_pending");
    const uint64_t n = rng.below(kMaxRows / 2);
    s.store.clear();
    for (uint64_t i = 0; i < n; ++i) s.store.push_back(Row{s.fresh(), s.fresh()});
    s.capacity = std::max(s.capacity, std::max<uint64_t>(n, 1));
    for (ModelOf* mo : {&s.m, &s.c, &s.h}) { mo->rows.assign((size_t)n, Held{}); mo->all = true; }
    s.d.replaced();
}

void op_lost(Sim& s, Rng& rng) {                                    // a device pass over the mirrors failed half way: no row of the store moved
    mutation(s);
    for (std::vector<uint64_t>* sh : {&s.s_m, &s.s_c})
        for (uint64_t& v : *sh) if (rng.one_in(2)) v = kGarbage;
    s.m.all = s.c.all = true;
    s.d.lost();
    s.just_lost = s.m.built;
}

void op_read(Sim& s, Rng& rng) {
    if (s.count() == 0) return;
    const bool all_current = s.d.bf16.current() && s.d.codes.current() && s.d.idtable.current() && s.s_m.size() >= s.capacity && s.s_c.size() >= s.capacity;
    const uint64_t which = rng.below(8);
    if (which == 0 || all_current) { read_bf16(s); read_codes(s); read_idtable(s); if (all_current) enter("reader_finds_everything_current"); return; }
    if (which < 3) read_bf16(s);
    else if (which < 4) read_idtable(s);
    else request(s, which < 7);
}

void run_sequence(uint64_t seed, uint64_t n_ops) {
    Rng rng(seed);
    Sim s(kSmallCap);
    g_seed = seed;
    for (g_op = 0; g_op < n_ops; ++g_op) {
        const uint64_t pick = rng.below(100);
        if (pick < 14) { g_what = "add batch"; op_add_batch(s, rng, false); }
        else if (pick < 20) { g_what = "overwrite burst"; op_add_batch(s, rng, true); }
        else if (pick < 22) { g_what = "overwrite alone"; if (s.count() > 0) { mutation(s); overwrite_row(s, rng.below(s.count())); } }   // (the engine says appended() first)
        else if (pick < 32) { g_what = "remove"; op_remove(s, rng); }
        else if (pick < 40) { g_what = "remove batch"; op_remove_batch(s, rng); }
        else if (pick < 42) { g_what = "replace"; op_replace(s, rng); }
        else if (pick < 44) { g_what = "lost"; op_lost(s, rng); }
        else if (pick < 47) { g_what = "reserve"; if (s.capacity < kMaxCapacity) s.capacity *= 2; }
        else { g_what = "a reader arrives"; op_read(s, rng); }
        // what may be read without a lock, after every operation
        CHECK(!s.d.bf16.current() || (s.m.built && s.m.to_convert() == 0), "a current bf16 fill has nothing to convert");
        CHECK(!s.d.codes.current() || (s.c.built && s.c.to_convert() == 0), "a current code fill has nothing to convert");
        CHECK(!s.d.idtable.current() || (s.h.built && s.h.to_convert() == 0), "a current id table has nothing to insert");
        const uint64_t probe = rng.below(s.count() + 2);
        CHECK(s.d.bf16.holds(probe) == s.m.holds(probe), "holds(" + std::to_string(probe) + ")");
    }
}

// The real cap, once: kMirrorMaxDirty overwrites are listed one by one, the next one starts the mirror over.
void run_real_cap() {
    g_seed = 0; g_op = 0; g_what = "the real cap";
    Sim s(kMirrorMaxDirty);
    Rng rng(7);
    s.d.appended();
    grow_store(s, kMirrorMaxDirty + 904);
    for (uint64_t i = 0; i < kMirrorMaxDirty + 904; ++i) append_row(s);
    read_bf16(s);
    s.d.appended();
    for (uint64_t i = 0; i < kMirrorMaxDirty; ++i) overwrite_row(s, i % 3 == 0 ? rng.below(s.count()) : i);
    CHECK(!s.d.bf16.restarting() && s.d.bf16.pending(s.count()) == kMirrorMaxDirty, "kMirrorMaxDirty overwrites are listed");
    read_bf16(s);
    s.d.appended();
    for (uint64_t i = 0; i <= kMirrorMaxDirty; ++i) overwrite_row(s, s.count() - 1 - i);
    CHECK(s.d.bf16.restarting() && s.d.bf16.pending(s.count()) == s.count(), "one more starts the mirror over");
    read_bf16(s);
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t n_seq = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 60;
    const uint64_t n_ops = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 600;
    const uint64_t seed0 = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 5201;
    for (uint64_t i = 0; i < n_seq; ++i) run_sequence(seed0 + i, n_ops);
    run_real_cap();
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
