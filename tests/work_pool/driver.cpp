// Stand-alone driver of wax_amd/csrc/work_pool.h (no HIP, no GPU): WorkPool<T> and TicketTable<T> against a model on one thread, then
// with real threads (at most 8). Every scenario that could block sits under a watchdog that fails the run instead of hanging it.
// Prints one `state NAME COUNT` line per state and a final `ok:` line; any violated invariant prints FAILED and exits 1.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <map>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "work_pool.h"

namespace {

const char* const kStates[] = {
    "reuse", "fresh_below_cap", "wait_woken_by_release", "try_refused", "holder_grows", "holder_refused_at_hard_cap", "make_fails_nothing_registered",
    "cap_raised_wakes_waiter", "cap_lowered_below_size", "for_each_sees_every_item_once", "deadlock_grow_both_return", "deadlock_try_both_refused",
    "threads_contended_wait", "ticket_ids_from_one", "ticket_taken_once_from_any_thread", "ticket_unknown_refused", "ticket_peek_leaves_it",
};
std::mutex g_state_mu;
std::map<std::string, unsigned long long> g_entered;
void enter(const std::string& s) { std::unique_lock<std::mutex> g(g_state_mu); g_entered[s] += 1; }

[[noreturn]] void die(const char* what, int line) {
    std::printf("FAILED: %s (line %d)\n", what, line);
    std::fflush(stdout);
    std::_Exit(1);
}
#define CHECK(c) do { if (!(c)) die(#c, __LINE__); } while (0)

// fails the run if it is still alive `secs` seconds later (it polls a flag: no timed wait on a condition variable, which the
// ThreadSanitizer runtime of some compilers does not follow)
class Watchdog {
public:
    Watchdog(const char* what, int secs) : t_([this, what, secs] {
        const auto t0 = std::chrono::steady_clock::now();
        while (!done_.load()) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(secs)) die(what, 0);
            std::this_thread::sleep_for(std::chrono::milliseconds(2));
        }
    }) {}
    ~Watchdog() { done_.store(true); t_.join(); }
private:
    std::atomic<bool> done_{false};
    std::thread t_;
};

struct Item {
    int index = -1;
    std::atomic<int> owners{0};
};
void own(Item* it) { CHECK(it->owners.fetch_add(1) == 0); }       // no item is handed to two owners
void disown(Item* it) { CHECK(it->owners.fetch_sub(1) == 1); }

constexpr int kMakeFailed = 7;
struct Maker {
    bool fail = false;
    int made = 0;
    int operator()(int index, Item** out) {
        if (fail) return kMakeFailed;
        *out = new Item();
        (*out)->index = index;
        ++made;
        return 0;
    }
};

void spin_until(const std::atomic<int>& a, int v) { while (a.load() < v) std::this_thread::yield(); }
void nap(int ms) { std::this_thread::sleep_for(std::chrono::milliseconds(ms)); }

// ---- one thread, against a model: `all` in the order of making, `free` as a stack -----------------------------------------------------
unsigned long long model_replay(uint32_t seed, int n_ops) {
    std::mt19937 rng(seed);
    const int hard = 6;
    int cap = 2 + (int)(rng() % 3);                       // 2 .. 4
    WorkPool<Item> pool(cap, hard);
    std::vector<Item*> all, free_, held;
    Maker mk;
    const bool seeded = rng() % 2;
    if (seeded) {                                         // the item created with the owner
        Item* it = new Item(); it->index = 0;
        pool.seed(it); all.push_back(it); free_.push_back(it);
    }
    for (int op = 0; op < n_ops; ++op) {
        const uint32_t what = rng() % 10;
        if (what < 5) {
            const bool would_block = free_.empty() && (int)all.size() >= cap;
            PoolMode mode = (PoolMode)(rng() % 3);
            if (mode == PoolMode::wait && would_block) mode = (rng() % 2) ? PoolMode::tries : PoolMode::grow;
            mk.fail = rng() % 8 == 0;
            Item* got = nullptr;
            int rc = 0;
            const PoolGot r = pool.acquire(mode, &got, &rc, mk);
            if (!free_.empty()) {
                CHECK(r == PoolGot::reused && got == free_.back());
                free_.pop_back(); held.push_back(got); own(got); enter("reuse");
            } else if ((int)all.size() < cap || (mode == PoolMode::grow && (int)all.size() < hard)) {
                if (mk.fail) {
                    CHECK(r == PoolGot::failed && rc == kMakeFailed && got == nullptr);
                    enter("make_fails_nothing_registered");
                } else {
                    CHECK(r == PoolGot::fresh && rc == 0 && got && got->index == (int)all.size());
                    enter((int)all.size() < cap ? "fresh_below_cap" : "holder_grows");
                    all.push_back(got); held.push_back(got); own(got);
                }
            } else if (mode == PoolMode::tries) {
                CHECK(r == PoolGot::busy && got == nullptr); enter("try_refused");
            } else {
                CHECK(mode == PoolMode::grow && r == PoolGot::exhausted && got == nullptr && (int)all.size() == hard);
                enter("holder_refused_at_hard_cap");
            }
        } else if (what < 8) {
            if (held.empty()) continue;
            const size_t i = rng() % held.size();
            Item* it = held[i];
            held.erase(held.begin() + (long)i);
            disown(it); pool.release(it); free_.push_back(it);
        } else if (what == 8) {
            cap = 1 + (int)(rng() % 4);
            pool.set_cap(cap);
            if (cap < (int)all.size()) enter("cap_lowered_below_size");
        } else {
            std::vector<Item*> seen;
            pool.for_each([&seen](Item* it) { seen.push_back(it); });
            CHECK(seen == all);                              // every item exactly once, in the order of making
            if (!all.empty()) enter("for_each_sees_every_item_once");
        }
        CHECK(pool.size() == all.size() && pool.cap() == cap && (int)pool.size() <= hard);
        CHECK(free_.size() + held.size() == all.size());    // free is a subset of all, and nothing is lost
    }
    for (Item* it : held) { disown(it); pool.release(it); }
    std::vector<Item*> drained;
    pool.drain([&drained](Item* it) { drained.push_back(it); });
    CHECK(drained == all && pool.size() == 0 && mk.made + (seeded ? 1 : 0) == (int)all.size());
    for (Item* it : drained) delete it;
    Item* after = nullptr;                                   // a drained pool has nothing idle: it would make one
    int rc = 0;
    mk.fail = true;
    pool.set_cap(1);
    CHECK(pool.acquire(PoolMode::tries, &after, &rc, mk) == PoolGot::failed && after == nullptr);
    return (unsigned long long)n_ops;
}

// ---- real threads ---------------------------------------------------------------------------------------------------------------------
void drain_delete(WorkPool<Item>& pool) { pool.drain([](Item* it) { delete it; }); }

// a waiter sleeps in PoolMode::wait until (a) a release, (b) a raised cap
void waiter_scenarios() {
    for (int raise = 0; raise < 2; ++raise) {
        Watchdog dog("a waiter was not woken", 20);
        WorkPool<Item> pool(2, 4);
        Maker mk;
        Item *a = nullptr, *b = nullptr;
        int rc = 0;
        CHECK(pool.acquire(PoolMode::wait, &a, &rc, mk) == PoolGot::fresh);
        CHECK(pool.acquire(PoolMode::wait, &b, &rc, mk) == PoolGot::fresh);
        own(a); own(b);
        std::atomic<int> stage{0};
        PoolGot got = PoolGot::failed;
        Item* c = nullptr;
        std::thread t([&] {
            Maker mine;
            int trc = 0;
            stage.store(1);
            got = pool.acquire(PoolMode::wait, &c, &trc, mine);
            own(c);
            stage.store(2);
        });
        spin_until(stage, 1);
        nap(20);
        CHECK(stage.load() == 1);                          // still waiting: both items are out and the cap is reached
        if (raise) pool.set_cap(3);
        else { disown(a); pool.release(a); }
        t.join();
        if (raise) { CHECK(got == PoolGot::fresh && c != a && c != b && pool.size() == 3); enter("cap_raised_wakes_waiter"); disown(a); pool.release(a); }
        else { CHECK(got == PoolGot::reused && c == a && pool.size() == 2); enter("wait_woken_by_release"); }
        disown(b); pool.release(b); disown(c); pool.release(c);
        drain_delete(pool);
    }
}

// The deadlock PoolMode::grow exists for: two threads hold half of the pool each and ask for one more. Waiting, each would wait for the
// other; growing, both return; trying, both are refused at once.
void deadlock_scenario(PoolMode mode) {
    Watchdog dog("two holders blocked each other", 20);
    WorkPool<Item> pool(4, 6);
    std::atomic<int> holding{0};
    PoolGot got[2] = {PoolGot::failed, PoolGot::failed};
    std::vector<std::thread> ts;
    for (int t = 0; t < 2; ++t)
        ts.emplace_back([&, t] {
            Maker mk;
            int rc = 0;
            Item *a = nullptr, *b = nullptr, *c = nullptr;
            CHECK(pool.acquire(PoolMode::wait, &a, &rc, mk) == PoolGot::fresh);
            CHECK(pool.acquire(PoolMode::wait, &b, &rc, mk) == PoolGot::fresh);
            own(a); own(b);
            holding.fetch_add(1);
            spin_until(holding, 2);                        // the pool is at its cap and nothing is free
            got[t] = pool.acquire(mode, &c, &rc, mk);
            if (c) own(c);
            holding.fetch_add(1);
            spin_until(holding, 4);                        // (neither releases before the other has its answer)
            if (c) { disown(c); pool.release(c); }
            disown(a); pool.release(a); disown(b); pool.release(b);
        });
    for (auto& t : ts) t.join();
    if (mode == PoolMode::grow) { CHECK(got[0] == PoolGot::fresh && got[1] == PoolGot::fresh && pool.size() == 6); enter("deadlock_grow_both_return"); }
    else { CHECK(got[0] == PoolGot::busy && got[1] == PoolGot::busy && pool.size() == 4); enter("deadlock_try_both_refused"); }
    drain_delete(pool);
}

// 8 threads on 3 items (hard cap 5): a thread with nothing waits or tries; one that holds an item asks for a second the way a ticket holder
// does — it grows or tries, never waits
void contended(int rounds) {
    Watchdog dog("the contended pool stalled", 60);
    WorkPool<Item> pool(3, 5);
    std::atomic<unsigned long long> waits{0};
    std::vector<std::thread> ts;
    for (int t = 0; t < 8; ++t)
        ts.emplace_back([&, t] {
            std::mt19937 rng(1234u + (uint32_t)t);
            Maker mk;
            for (int i = 0; i < rounds; ++i) {
                int rc = 0;
                Item *a = nullptr, *b = nullptr;
                const bool wait = rng() % 4 != 0;
                const PoolGot r = pool.acquire(wait ? PoolMode::wait : PoolMode::tries, &a, &rc, mk);
                if (r == PoolGot::busy) continue;
                CHECK(r == PoolGot::reused || r == PoolGot::fresh);
                own(a);
                if (wait) waits.fetch_add(1);
                if (rng() % 3 == 0) {
                    const PoolGot r2 = pool.acquire((rng() % 2) ? PoolMode::grow : PoolMode::tries, &b, &rc, mk);
                    CHECK(r2 != PoolGot::failed);
                    if (b) own(b);
                }
                CHECK(pool.size() <= 5);
                if (rng() % 8 == 0) std::this_thread::yield();
                if (b) { disown(b); pool.release(b); }
                disown(a); pool.release(a);
            }
        });
    for (auto& t : ts) t.join();
    size_t n = 0;
    pool.for_each([&n](Item* it) { CHECK(it->owners.load() == 0); ++n; });
    CHECK(n == pool.size() && n >= 3 && n <= 5);
    if (waits.load() > 0) enter("threads_contended_wait");
    drain_delete(pool);
}

void tickets() {
    {
        TicketTable<int> t;
        CHECK(t.empty());
        CHECK(t.put(10) == 1 && t.put(20) == 2 && t.put(30) == 3 && !t.empty());
        enter("ticket_ids_from_one");
        int v = 0, seen = 0;
        CHECK(t.peek(2, [&seen](const int& x) { seen = x; }) && seen == 20 && t.peek(2, [](const int&) {}));
        enter("ticket_peek_leaves_it");
        CHECK(t.take(2, &v) && v == 20 && !t.take(2, &v) && !t.peek(2, [](const int&) {}) && !t.take(0, &v) && !t.take(4, &v));
        enter("ticket_unknown_refused");
        CHECK(t.put(40) == 4);                             // never reused
        CHECK(t.take(1, &v) && v == 10 && t.take(3, &v) && v == 30 && t.take(4, &v) && v == 40 && t.empty());
    }
    Watchdog dog("the ticket threads stalled", 60);
    constexpr int kThreads = 8, kPer = 2000, kTotal = kThreads * kPer;
    TicketTable<int> table;
    std::vector<std::atomic<int>> taken(kTotal + 2);
    for (auto& a : taken) a.store(0);
    std::atomic<int> stage{0};
    std::vector<std::thread> ts;
    for (int t = 0; t < kThreads; ++t)
        ts.emplace_back([&, t] {
            uint64_t last = 0;
            for (int i = 0; i < kPer; ++i) {
                const uint64_t id = table.put(t);
                CHECK(id > last && id >= 1 && id <= (uint64_t)kTotal);   // strictly increasing, as every thread sees them
                last = id;
            }
            stage.fetch_add(1);
            spin_until(stage, kThreads);
            // every thread goes for every id, starting somewhere else: exactly one take per id succeeds, whoever put it
            for (int i = 0; i < kTotal + 2; ++i) {
                const int id = (i + t * kPer) % (kTotal + 2);
                int v = -1;
                if (table.take((uint64_t)id, &v)) { CHECK(v >= 0 && v < kThreads); taken[(size_t)id].fetch_add(1); }
            }
        });
    for (auto& t : ts) t.join();
    CHECK(taken[0].load() == 0 && taken[kTotal + 1].load() == 0 && table.empty());
    for (int id = 1; id <= kTotal; ++id) CHECK(taken[(size_t)id].load() == 1);
    enter("ticket_taken_once_from_any_thread");
}

}  // namespace

int main() {
    unsigned long long n_ops = 0, n_seq = 0;
    for (uint32_t seed = 1; seed <= 300; ++seed, ++n_seq) n_ops += model_replay(seed, 400);
    waiter_scenarios();
    deadlock_scenario(PoolMode::grow);
    deadlock_scenario(PoolMode::tries);
    contended(4000);
    tickets();
    bool ok = true;
    for (const char* name : kStates) {
        std::printf("state %s %llu\n", name, g_entered[name]);
        if (g_entered[name] == 0) ok = false;
    }
    for (const auto& kv : g_entered)
        if (std::find(std::begin(kStates), std::end(kStates), kv.first) == std::end(kStates)) {
            std::printf("FAILED: state %s is entered but not listed\n", kv.first.c_str());
            ok = false;
        }
    if (!ok) { std::printf("FAILED: a state was never entered\n"); return 1; }
    std::printf("ok: %llu sequences of %llu operations, %zu states\n", n_seq, n_ops, std::size(kStates));
    return 0;
}
