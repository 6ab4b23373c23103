// Stand-alone driver of wax_amd/csrc/rw_lock.h (no HIP, no GPU): RWLock, WriteGuard and TicketHolders with real threads (at most 8).
// Every scenario sits under a watchdog that fails the run instead of hanging it. Prints one `state NAME COUNT` line per state and a
// final `ok:` line; any violated expectation prints FAILED and exits 1.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <string>
#include <thread>
#include <vector>

#include "rw_lock.h"

namespace {

const char* const kStates[] = {
    "holder_reenters_past_queued_writer", "reader_without_ticket_queues_behind_writer", "writer_excludes_readers", "unlock_from_another_thread",
    "epoch_constant_under_shared_lock", "epoch_advances_by_one_per_writer", "holding_drops_when_another_thread_collects", "reader_waits_for_active_writer", "threads_mixed",
};
unsigned long long g_entered[std::size(kStates)] = {};
void enter(const char* name) {   // (called from the main thread only)
    for (size_t i = 0; i < std::size(kStates); ++i)
        if (std::string(kStates[i]) == name) { g_entered[i] += 1; return; }
    std::printf("FAILED: state %s is entered but not listed\n", name);
    std::_Exit(1);
}

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

void spin_until(const std::atomic<int>& a, int v) { while (a.load() < v) std::this_thread::yield(); }
void nap(int ms) { std::this_thread::sleep_for(std::chrono::milliseconds(ms)); }

// The deadlock the `reentrant` flag exists for. The main thread holds a ticket (= the shared lock). A writer queues. A reader without a
// ticket queues behind the writer. The main thread submits again: with holding() > 0 it re-enters at once — queued behind the writer it
// would wait for a writer that waits for it. Then it collects both: the writer runs alone, then the plain reader.
void reentry_scenario() {
    Watchdog dog("a ticket holder did not get past the queued writer", 20);
    RWLock lock;
    TicketHolders holders;
    std::thread::id owner1, owner2;
    CHECK(holders.holding() == 0);
    lock.lock_shared(holders.holding() > 0);
    holders.note_submit(&owner1);
    const uint64_t e0 = lock.epoch();

    std::atomic<int> w_stage{0}, r_stage{0}, readers_in{0};
    bool reader_was_out = false;
    uint64_t e_writer = 0;
    std::thread writer([&] {
        w_stage.store(1);
        WriteGuard w(lock);
        e_writer = lock.epoch();
        reader_was_out = readers_in.load() == 0 && r_stage.load() == 1;   // the plain reader asked before and is still outside
        w_stage.store(2);
        nap(5);
        reader_was_out = reader_was_out && readers_in.load() == 0;
    });
    spin_until(w_stage, 1);
    nap(60);                                                   // (long enough for the writer to have queued, on a loaded machine too)
    CHECK(w_stage.load() == 1);                                // the writer waits for the ticket to be collected
    std::thread reader([&] {
        CHECK(holders.holding() == 0);
        r_stage.store(1);
        lock.lock_shared(holders.holding() > 0);
        readers_in.fetch_add(1);
        CHECK(w_stage.load() == 2);                            // only after the writer
        r_stage.store(2);
        lock.unlock_shared();
    });
    spin_until(r_stage, 1);
    nap(20);
    CHECK(r_stage.load() == 1 && readers_in.load() == 0);      // queued behind the waiting writer
    CHECK(holders.holding() == 1);
    lock.lock_shared(holders.holding() > 0);                   // returns: this is the state
    holders.note_submit(&owner2);
    CHECK(holders.holding() == 2 && w_stage.load() == 1 && r_stage.load() == 1);
    enter("holder_reenters_past_queued_writer");
    CHECK(lock.epoch() == e0);
    enter("epoch_constant_under_shared_lock");
    holders.note_collect(owner1); lock.unlock_shared();
    holders.note_collect(owner2); lock.unlock_shared();
    writer.join();
    reader.join();
    CHECK(holders.holding() == 0);
    CHECK(reader_was_out);
    enter("writer_excludes_readers");
    CHECK(r_stage.load() == 2);
    enter("reader_without_ticket_queues_behind_writer");
    CHECK(e_writer == e0 + 1 && lock.epoch() == e0 + 1);
    for (int i = 0; i < 5; ++i) { WriteGuard w(lock); }
    CHECK(lock.epoch() == e0 + 6);
    enter("epoch_advances_by_one_per_writer");
}

// A ticket submitted on one thread is collected on another: the shared lock is released there, and the submitter's count drops.
void handover_scenario() {
    Watchdog dog("a lock released by another thread stayed held", 20);
    RWLock lock;
    TicketHolders holders;
    std::thread::id owner_a, owner_b;
    std::atomic<int> stage{0};
    int held_by_submitter[3] = {-1, -1, -1};
    std::thread submitter([&] {
        lock.lock_shared(holders.holding() > 0); holders.note_submit(&owner_a);
        lock.lock_shared(holders.holding() > 0); holders.note_submit(&owner_b);
        held_by_submitter[0] = holders.holding();
        stage.store(1);
        spin_until(stage, 2);
        held_by_submitter[1] = holders.holding();
        spin_until(stage, 3);
        held_by_submitter[2] = holders.holding();
    });
    spin_until(stage, 1);
    CHECK(holders.holding() == 0);                             // the collecting thread holds nothing of its own
    holders.note_collect(owner_a); lock.unlock_shared();
    stage.store(2);
    nap(1);
    holders.note_collect(owner_b); lock.unlock_shared();
    stage.store(3);
    submitter.join();
    CHECK(held_by_submitter[0] == 2 && held_by_submitter[2] == 0 && (held_by_submitter[1] == 1 || held_by_submitter[1] == 0));
    enter("holding_drops_when_another_thread_collects");
    { WriteGuard w(lock); }                                    // both shared locks are gone: a writer gets in
    lock.lock();
    std::thread other([&] { lock.unlock(); });
    other.join();
    lock.lock_shared();
    lock.unlock_shared();
    enter("unlock_from_another_thread");
    // an active writer with no other writer queued: a reader waits for it, a ticket holder too (it cannot be one: the writer got in)
    for (int reentrant = 0; reentrant < 2; ++reentrant) {
        lock.lock();
        std::atomic<int> r_stage{0};
        std::thread reader([&] {
            r_stage.store(1);
            lock.lock_shared(reentrant != 0);
            r_stage.store(2);
            lock.unlock_shared();
        });
        spin_until(r_stage, 1);
        nap(20);
        CHECK(r_stage.load() == 1);
        lock.unlock();
        reader.join();
        enter("reader_waits_for_active_writer");
    }
}

// 6 readers and 2 writers on two plain counters that only agree outside a writer's section; a reader that holds a ticket submits again
// the way a pipelining caller does, while writers queue
void mixed(int rounds) {
    Watchdog dog("the mixed readers and writers stalled", 60);
    RWLock lock;
    TicketHolders holders;
    long x = 0, y = 0;                                          // guarded by `lock`
    std::vector<std::thread> ts;
    for (int t = 0; t < 8; ++t)
        ts.emplace_back([&, t] {
            for (int i = 0; i < rounds; ++i) {
                if (t < 2) {
                    WriteGuard w(lock);
                    ++x; ++y;
                } else {
                    std::thread::id o1, o2;
                    lock.lock_shared(holders.holding() > 0); holders.note_submit(&o1);
                    const uint64_t e = lock.epoch();
                    CHECK(x == y);
                    if ((i + t) % 3 == 0) {
                        lock.lock_shared(holders.holding() > 0); holders.note_submit(&o2);
                        CHECK(x == y && lock.epoch() == e);
                        holders.note_collect(o2); lock.unlock_shared();
                    }
                    CHECK(lock.epoch() == e);
                    holders.note_collect(o1); lock.unlock_shared();
                    CHECK(holders.holding() == 0);
                }
            }
        });
    for (auto& t : ts) t.join();
    CHECK(x == 2L * rounds && y == x && lock.epoch() == (uint64_t)(2 * rounds));
    enter("threads_mixed");
}

}  // namespace

int main() {
    reentry_scenario();
    handover_scenario();
    mixed(3000);
    bool ok = true;
    for (size_t i = 0; i < std::size(kStates); ++i) {
        std::printf("state %s %llu\n", kStates[i], g_entered[i]);
        if (g_entered[i] == 0) ok = false;
    }
    if (!ok) { std::printf("FAILED: a state was never entered\n"); return 1; }
    std::printf("ok: 3 scenarios, %zu states\n", std::size(kStates));
    return 0;
}
