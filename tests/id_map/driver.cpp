// Stand-alone driver of wax_amd/csrc/id_map.h (no HIP, no GPU): IdMap against std::unordered_map. Aimed probe clusters in a 1 024-slot
// table — ids chosen by their home slot, clusters that wrap round the end of the table included —, the cases of renumber_removed's
// word-aligned bitmap, and seeded random sequences of a store's operations. Prints one `state NAME COUNT` line per state and a final
// `ok:` line; any disagreement with the model prints FAILED and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <map>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include "id_map.h"

namespace {

const char* const kStates[] = {
    "overwrite_present", "growth_and_rehash", "erase_absent", "erase_cluster_head", "erase_cluster_middle", "erase_cluster_tail",
    "wrap_erase_before_the_end", "wrap_erase_after_the_start", "wrap_mixed_homes", "reserve_spares_growth", "clear_empties",
    "renumber_first_on_word_boundary", "renumber_first_off_word_boundary", "renumber_last_row", "renumber_single_row", "renumber_whole_word",
    "renumber_three_words_one_empty", "renumber_nothing", "erase_row_renumbers", "store_of_100000_rows",
};
std::map<std::string, unsigned long long> g_entered;
void enter(const std::string& s) { g_entered[s] += 1; }

[[noreturn]] void die(const char* what, int line) {
    std::printf("FAILED: %s (line %d)\n", what, line);
    std::fflush(stdout);
    std::_Exit(1);
}
#define CHECK(c) do { if (!(c)) die(#c, __LINE__); } while (0)

using Model = std::unordered_map<uint64_t, uint32_t>;
void agree(const IdMap& m, const Model& model) {
    CHECK(m.size() == model.size());
    for (const auto& kv : model) CHECK(m.find(kv.first) == (int64_t)kv.second);
}

// ids by home slot in a table of `slots` slots: the n-th id (from 1 up) whose home is `home`
std::vector<uint64_t> ids_at_home(size_t home, size_t slots, size_t n, uint64_t from = 1) {
    std::vector<uint64_t> out;
    for (uint64_t id = from; out.size() < n; ++id)
        if ((IdMap::hash(id) & (slots - 1)) == home) out.push_back(id);
    return out;
}

// ---- probe clusters --------------------------------------------------------------------------------------------------------------------
// `homes[i]` is the home slot of the i-th inserted entry, relative to `base` (cyclically). Erase each entry in turn from a fresh table,
// by both erasing calls, and hold the rest to the model; put it back and look again.
void cluster(size_t base, const std::vector<int>& homes, bool same_home) {
    const size_t slots = 1024;
    std::vector<uint64_t> ids;
    std::map<size_t, uint64_t> next_from;
    for (int h : homes) {
        const size_t home = (base + (size_t)h) & (slots - 1);
        uint64_t& from = next_from[home];
        const uint64_t id = ids_at_home(home, slots, 1, from + 1)[0];
        from = id;
        ids.push_back(id);
    }
    const bool wraps = base + homes.size() > slots;          // same home: the entries lie in consecutive slots from `base`; mixed homes at these bases: some entry lies behind the end
    for (size_t p = 0; p < ids.size(); ++p)
        for (int how = 0; how < 2; ++how) {
            IdMap m;
            Model model;
            CHECK(m.slots() == slots);
            for (size_t i = 0; i < ids.size(); ++i) { m.put(ids[i], (uint32_t)(10 + i)); model[ids[i]] = (uint32_t)(10 + i); }
            agree(m, model);
            if (how == 0) { m.erase_only(ids[p]); model.erase(ids[p]); }
            else {
                m.erase_row(ids[p], (uint32_t)(10 + p)); model.erase(ids[p]);
                for (auto& kv : model) if (kv.second > 10 + p) kv.second -= 1;
                enter("erase_row_renumbers");
            }
            CHECK(m.find(ids[p]) == -1);
            agree(m, model);
            m.erase_only(ids[p]);                            // absent now: nothing changes
            agree(m, model);
            enter("erase_absent");
            m.put(ids[p], 7u); model[ids[p]] = 7u;
            agree(m, model);
            for (uint64_t id : ids) { m.erase_only(id); model.erase(id); agree(m, model); }
            CHECK(m.size() == 0);
            if (same_home) {                                 // the p-th inserted entry lies in slot base + p
                enter(p == 0 ? "erase_cluster_head" : p + 1 == ids.size() ? "erase_cluster_tail" : "erase_cluster_middle");
                if (wraps) enter(base + p < slots ? "wrap_erase_before_the_end" : "wrap_erase_after_the_start");
            } else if (wraps) {
                enter("wrap_mixed_homes");
            }
        }
}

void clusters() {
    std::mt19937 rng(99);
    for (size_t base : {(size_t)500, (size_t)1021, (size_t)1022, (size_t)1023}) {
        cluster(base, {0, 0, 0, 0, 0, 0, 0}, /*same_home=*/true);
        for (int rep = 0; rep < 40; ++rep) {                 // homes in {base, base + 1, base + 2, base + 3}, 5 .. 9 entries
            std::vector<int> homes(5 + rng() % 5);
            for (int& h : homes) h = (int)(rng() % 4);
            homes[0] = 0;
            cluster(base, homes, /*same_home=*/false);
        }
    }
}

// ---- a store: row r holds ids[r] ------------------------------------------------------------------------------------------------------
struct Store {
    IdMap m;
    std::vector<uint64_t> ids;
    void check() const {
        CHECK(m.size() == ids.size());
        for (size_t r = 0; r < ids.size(); ++r) CHECK(m.find(ids[r]) == (int64_t)r);
    }
    void append(uint64_t id) { m.put(id, (uint32_t)ids.size()); ids.push_back(id); }
    void remove_batch(const std::vector<uint32_t>& rem) {   // ascending, distinct
        const uint64_t rows = ids.size();
        std::vector<uint64_t> gone;
        for (uint32_t r : rem) { m.erase_only(ids[r]); gone.push_back(ids[r]); }
        m.renumber_removed(rem, rows);
        std::vector<uint64_t> kept;
        for (uint32_t r = 0; r < rows; ++r) if (!std::binary_search(rem.begin(), rem.end(), r)) kept.push_back(ids[r]);
        ids.swap(kept);
        for (uint64_t id : gone) CHECK(m.find(id) == -1);
        check();
    }
};

void renumber_case(const char* state, uint32_t rows, const std::vector<uint32_t>& rem) {
    Store s;
    for (uint32_t r = 0; r < rows; ++r) s.append(0x1000u + 3u * r);
    s.check();
    s.remove_batch(rem);
    enter(state);
}

void renumber_cases() {
    auto range = [](uint32_t lo, uint32_t hi) { std::vector<uint32_t> v; for (uint32_t r = lo; r < hi; ++r) v.push_back(r); return v; };
    renumber_case("renumber_first_on_word_boundary", 300, {64, 65, 130});
    renumber_case("renumber_first_on_word_boundary", 300, {0, 299});
    renumber_case("renumber_first_off_word_boundary", 300, {70, 71, 127, 128, 191, 192});
    renumber_case("renumber_first_off_word_boundary", 300, {63, 64});
    renumber_case("renumber_last_row", 300, {299});
    renumber_case("renumber_last_row", 128, {127});
    renumber_case("renumber_last_row", 129, {128});
    renumber_case("renumber_last_row", 129, {5, 127, 128});
    renumber_case("renumber_single_row", 300, {150});
    renumber_case("renumber_single_row", 1, {0});
    renumber_case("renumber_whole_word", 300, range(64, 128));
    renumber_case("renumber_whole_word", 256, range(0, 256));
    renumber_case("renumber_three_words_one_empty", 300, {70, 100, 200, 260});
    renumber_case("renumber_three_words_one_empty", 320, {1, 63, 128, 129, 319});
    renumber_case("renumber_nothing", 300, {});
}

unsigned long long random_store(uint32_t seed, int n_ops) {
    std::mt19937_64 rng(seed);
    Store s;
    uint64_t next_id = 1 + (rng() % 1000);
    auto fresh = [&] { next_id += 1 + rng() % ((seed % 3 == 0) ? 3 : 1000000007ull); return next_id; };   // dense ids and scattered ones
    for (int op = 0; op < n_ops; ++op) {
        const uint32_t what = (uint32_t)(rng() % 100);
        const size_t n = s.ids.size();
        if (what < 45 || n == 0) {
            if (n < 400) s.append(fresh());
        } else if (what < 55) {
            const size_t r = rng() % n;
            s.m.put(s.ids[r], (uint32_t)r);                  // an upsert: the id keeps its row
            enter("overwrite_present");
        } else if (what < 70) {
            const uint32_t r = (uint32_t)(rng() % n);
            s.m.erase_row(s.ids[r], r);
            s.ids.erase(s.ids.begin() + r);
            enter("erase_row_renumbers");
        } else if (what < 75) {
            s.m.erase_only(next_id + 12345);
            CHECK(s.m.find(next_id + 12345) == -1);
            enter("erase_absent");
        } else if (what < 92) {
            std::vector<uint32_t> rem;
            const size_t want = 1 + rng() % 20;
            for (uint32_t r = 0; r < n; ++r) if (rng() % n < want) rem.push_back(r);
            s.remove_batch(rem);
            if (rem.empty()) enter("renumber_nothing");
        } else if (what < 97) {
            const size_t before = s.m.slots();
            s.m.reserve(rng() % 3000);
            CHECK(s.m.slots() >= before);
        } else {
            s.m.clear(); s.ids.clear();
            CHECK(s.m.size() == 0 && s.m.slots() == 1024 && s.m.find(next_id) == -1);
            enter("clear_empties");
        }
        s.check();
    }
    return (unsigned long long)n_ops;
}

// put / find / erase_only with values that are no rows: an overwrite changes the value
void free_form(uint32_t seed) {
    std::mt19937_64 rng(seed);
    IdMap m;
    Model model;
    for (int op = 0; op < 6000; ++op) {
        const uint64_t id = rng() % 1500;                    // few ids: overwrites and erasures of present ids are common
        const uint32_t what = (uint32_t)(rng() % 10);
        if (what < 6) {
            const uint32_t v = (uint32_t)rng();
            if (model.count(id)) enter("overwrite_present");
            m.put(id, v); model[id] = v;
        } else if (what < 9) {
            if (!model.count(id)) enter("erase_absent");
            m.erase_only(id); model.erase(id);
        } else {
            CHECK(m.find(id) == (model.count(id) ? (int64_t)model[id] : -1));
        }
        if (op % 64 == 0) agree(m, model);
    }
    agree(m, model);
}

void growth() {
    {
        IdMap m;
        Model model;
        size_t slots = m.slots(), rehashes = 0;
        for (uint64_t i = 0; i < 5000; ++i) {
            m.put(i * 7919u, (uint32_t)i); model[i * 7919u] = (uint32_t)i;
            if (m.slots() != slots) { CHECK(m.slots() == 2 * slots); slots = m.slots(); ++rehashes; agree(m, model); enter("growth_and_rehash"); }
            CHECK(m.size() * 10 <= m.slots() * 6);           // the load the table promises its probes
        }
        CHECK(rehashes == 4);                                // 1 024 -> 16 384 slots for 5 000 ids
        agree(m, model);
    }
    {
        IdMap m;
        m.reserve(5000);
        const size_t slots = m.slots();
        CHECK(slots == 16384);
        for (uint64_t i = 0; i < 5000; ++i) m.put(i + 1, (uint32_t)i);
        CHECK(m.slots() == slots && m.size() == 5000);
        m.reserve(10);                                       // never shrinks
        CHECK(m.slots() == slots && m.find(5000) == 4999);
        enter("reserve_spares_growth");
    }
    {
        Store s;
        for (uint32_t r = 0; r < 100000; ++r) s.append(0x9e3779b97f4a7c15ull * (r + 1));
        CHECK(s.m.slots() == 262144);
        s.check();
        std::vector<uint32_t> rem;
        for (uint32_t r = 31; r < 100000; r += 97) rem.push_back(r);
        rem.push_back(99999);
        s.remove_batch(rem);
        s.m.erase_row(s.ids[500], 500); s.ids.erase(s.ids.begin() + 500);
        s.check();
        enter("store_of_100000_rows");
    }
}

}  // namespace

int main() {
    clusters();
    renumber_cases();
    growth();
    unsigned long long n_ops = 0, n_seq = 0;
    for (uint32_t seed = 1; seed <= 24; ++seed, ++n_seq) n_ops += random_store(seed, 1500);
    for (uint32_t seed = 1; seed <= 8; ++seed) free_form(seed);
    bool ok = true;
    for (const char* name : kStates) {
        std::printf("state %s %llu\n", name, g_entered[name]);
        if (g_entered[name] == 0) ok = false;
    }
    for (const auto& kv : g_entered)
        if (std::find_if(std::begin(kStates), std::end(kStates), [&](const char* s) { return kv.first == s; }) == std::end(kStates)) {
            std::printf("FAILED: state %s is entered but not listed\n", kv.first.c_str());
            ok = false;
        }
    if (!ok) { std::printf("FAILED: a state was never entered\n"); return 1; }
    std::printf("ok: %llu sequences of %llu operations, %zu states\n", n_seq, n_ops, std::size(kStates));
    return 0;
}
