// Stand-alone driver of wax_amd/csrc/shard_workers.h (no HIP, no GPU): the hand-off of jobs to 2 and to 8 persistent workers, from one
// caller and from three at once, with workers found polling (back-to-back jobs), found asleep (pauses longer than kSpinUs) and outlasting
// the caller's own polling (a job longer than kSpinUs). Everything sits under a watchdog that fails the run instead of hanging it.
// Prints one `state NAME COUNT` line per state and a final `ok:` line; any violated expectation prints FAILED and exits 1.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "shard_workers.h"

namespace {

const char* const kStates[] = {
    "burst_workers_polling", "pause_workers_asleep", "long_job_caller_sleeps", "three_callers_at_once", "try_refused_while_long_job_runs",
    "try_runs_when_free", "stop_while_asleep", "stop_while_polling", "stop_before_any_job", "on_start_once_per_worker",
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

class Watchdog {   // fails the run if it is still alive `secs` seconds later
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

void nap_us(int us) { std::this_thread::sleep_for(std::chrono::microseconds(us)); }
constexpr int kPauseUs = 5 * ShardWorkers::kSpinUs;   // well past the workers' polling: they are asleep afterwards
std::atomic<unsigned long long> g_handoffs{0};

struct Crew {
    size_t n;
    std::unique_ptr<std::atomic<int>[]> started;
    ShardWorkers workers;
    explicit Crew(size_t n_) : n(n_), started(new std::atomic<int>[n_]) {
        for (size_t g = 0; g < n; ++g) started[g].store(0);
        workers.start(n, [this](size_t g) { started[g].fetch_add(1); });
    }
    // one job: it runs exactly once on every worker, and all of it has happened when run_all returns
    void job(int work_us, bool try_it = false) {
        std::unique_ptr<std::atomic<int>[]> hits(new std::atomic<int>[n]);
        for (size_t g = 0; g < n; ++g) hits[g].store(0);
        std::vector<long> plain(n, 0);                      // written without atomics: run_all's return orders it
        const std::function<void(size_t)> fn = [&](size_t g) {
            if (work_us > 0) nap_us(work_us);
            plain[g] += 1;
            hits[g].fetch_add(1);
        };
        if (try_it) CHECK(workers.try_run_all(fn));
        else workers.run_all(fn);
        for (size_t g = 0; g < n; ++g) CHECK(hits[g].load() == 1 && plain[g] == 1);
        g_handoffs.fetch_add(1);
    }
    void stop_and_check() {
        workers.stop();
        for (size_t g = 0; g < n; ++g) CHECK(started[g].load() == 1);
    }
};

void phases(size_t n) {
    Watchdog dog("a hand-off to the workers stalled", 120);
    {
        Crew c(n);
        for (int i = 0; i < 1500; ++i) c.job(0);             // back to back: the workers are found polling
        enter("burst_workers_polling");
        for (int i = 0; i < 25; ++i) { nap_us(kPauseUs); c.job(0); }
        enter("pause_workers_asleep");
        for (int i = 0; i < 5; ++i) c.job(kPauseUs);         // longer than the caller polls: it sleeps until the last worker reports
        enter("long_job_caller_sleeps");
        for (int i = 0; i < 10; ++i) { nap_us(kPauseUs); c.job(0); c.job(0); c.job(kPauseUs); c.job(0); }

        // three callers at once (this thread and two more): bursts, pauses and long jobs interleave; callers queue for the workers
        std::vector<std::thread> callers;
        auto caller = [&c](int t) {
            for (int i = 0; i < 300; ++i) {
                if ((i + t) % 50 == 0) nap_us(kPauseUs);
                c.job((i + 7 * t) % 97 == 0 ? kPauseUs : 0);
            }
        };
        for (int t = 1; t < 3; ++t) callers.emplace_back(caller, t);
        caller(0);
        for (auto& t : callers) t.join();
        enter("three_callers_at_once");

        // try_run_all: false at once while a long job holds the workers, true otherwise
        std::atomic<int> long_running{0};
        std::atomic<bool> let_go{false};
        std::thread holder([&] {
            const std::function<void(size_t)> fn = [&](size_t) {
                long_running.fetch_add(1);
                while (!let_go.load()) nap_us(100);
            };
            c.workers.run_all(fn);
        });
        while (long_running.load() < (int)n) std::this_thread::yield();
        int ran = 0;
        const std::function<void(size_t)> probe = [&ran](size_t) { ++ran; };
        const auto t0 = std::chrono::steady_clock::now();
        CHECK(!c.workers.try_run_all(probe) && ran == 0);
        CHECK(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(5));
        enter("try_refused_while_long_job_runs");
        let_go.store(true);
        holder.join();
        c.job(0, /*try_it=*/true);
        nap_us(kPauseUs);
        c.job(0, /*try_it=*/true);
        enter("try_runs_when_free");

        nap_us(kPauseUs);
        c.stop_and_check();                                  // every worker is asleep
        enter("stop_while_asleep");
        enter("on_start_once_per_worker");
    }
    for (int i = 0; i < 20; ++i) {
        Crew c(n);
        for (int j = 0; j < 3; ++j) c.job(0);
        c.stop_and_check();                                  // at once behind a job: the workers are polling
    }
    enter("stop_while_polling");
    {
        Crew c(n);
        c.stop_and_check();
        enter("stop_before_any_job");
    }
}

}  // namespace

int main() {
    phases(2);
    phases(8);
    bool ok = true;
    for (size_t i = 0; i < std::size(kStates); ++i) {
        std::printf("state %s %llu\n", kStates[i], g_entered[i]);
        if (g_entered[i] == 0) ok = false;
    }
    if (!ok) { std::printf("FAILED: a state was never entered\n"); return 1; }
    std::printf("ok: %llu hand-offs to 2 and to 8 workers, %zu states\n", g_handoffs.load(), std::size(kStates));
    return 0;
}
