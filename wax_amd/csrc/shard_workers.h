// shard_workers.h — the persistent per-shard host threads of a sharded handle and their hand-off. Plain C++17 over the standard
// library: no HIP and no project header — what ties a worker to its device is the callable given to start(). tests/shard_workers/driver.cpp
// runs the hand-off on the CPU, workers polling and workers asleep, also under ThreadSanitizer.
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

// A spin-wait hint, per architecture. It lives here because the workers' polling is its main user; the single-device collect
// (api_search.inc: the completion-word poll) spins with it too.
inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    std::this_thread::yield();
#endif
}

// Persistent per-shard worker threads: per-shard host work (single-query submits — one kernel launch each —, filtered search,
// the k > 192 batched path, mirror builds) runs on all shards at once without creating a thread per call. Worker g is bound
// to device g for its whole life.
// Hand-off (round 5): a job is published by bumping an atomic epoch; a worker that has just finished a job POLLS the epoch for
// kSpinUs before it goes back to sleep on the condition variable, and the caller polls the completion count the same way. While
// queries keep coming, a fan-out therefore costs an atomic store, the workers' own work side by side and an atomic load — not a
// futex wake per shard (5 - 10 us each) and not G launches one after the other from one thread (12 - 15 us per shard measured in
// round 4: 100 - 130 us per query at 8 shards). An idle handle burns no CPU: every worker is asleep kSpinUs after the last job.
class ShardWorkers {
  public:
    static constexpr int kSpinUs = 200;
    // n workers; worker g calls on_start(g) once, on its own thread, before its first job (the engine: bind the thread to device g)
    template <typename OnStart>
    void start(size_t n, OnStart on_start) {
        n_ = n;
        for (size_t g = 0; g < n_; ++g)
            threads_.emplace_back([this, g, on_start]() {
                on_start(g);
                uint64_t seen = 0;
                for (;;) {
                    // poll, then sleep
                    bool got = false;
                    const auto t0 = std::chrono::steady_clock::now();
                    for (uint32_t spins = 1;; ++spins) {
                        if (epoch_.load(std::memory_order_acquire) != seen || stop_.load(std::memory_order_acquire)) { got = true; break; }
                        cpu_relax();
                        if ((spins & 0xffu) == 0u &&
                            std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > kSpinUs)
                            break;
                    }
                    if (!got) {
                        std::unique_lock<std::mutex> lk(mu_);
                        ++sleepers_;
                        cv_.wait(lk, [&] { return stop_.load() || epoch_.load() != seen; });
                        --sleepers_;
                    }
                    if (stop_.load()) return;
                    seen = epoch_.load(std::memory_order_acquire);
                    const std::function<void(size_t)>* job = job_.load(std::memory_order_acquire);
                    (*job)(g);
                    // The last worker ALWAYS takes the mutex and notifies (one uncontended lock per job). Round 5 skipped this unless a
                    // `waiting_` flag was up — a store-then-load on both sides that release / acquire does not order: the caller could
                    // raise the flag, read done_ == n - 1 and go to sleep while the last worker read the flag as still down and never
                    // notified (advisor, round 5). Under the mutex the caller's predicate check and this notify cannot interleave that way.
                    if (done_.fetch_add(1, std::memory_order_acq_rel) + 1 == n_) {
                        std::unique_lock<std::mutex> lk(mu_);
                        done_cv_.notify_all();
                    }
                }
            });
    }
    // fn(g) on every worker, concurrently; returns when all are done. One job at a time per handle (callers queue here).
    void run_all(const std::function<void(size_t)>& fn) {
        std::unique_lock<std::mutex> one(job_mu_);
        run_locked(fn);
    }
    // The same, unless another job holds the workers (a mirror build, a filtered search, a k > 192 batch: milliseconds): then false at
    // once, and the caller does its short per-shard work itself instead of queueing behind the long job (advisor, round 5).
    bool try_run_all(const std::function<void(size_t)>& fn) {
        std::unique_lock<std::mutex> one(job_mu_, std::try_to_lock);
        if (!one.owns_lock()) return false;
        run_locked(fn);
        return true;
    }

  private:
    void run_locked(const std::function<void(size_t)>& fn) {
        job_.store(&fn, std::memory_order_release);
        done_.store(0, std::memory_order_release);
        epoch_.fetch_add(1, std::memory_order_acq_rel);
        {
            std::unique_lock<std::mutex> lk(mu_);    // (a worker checks the epoch under this lock before it sleeps: no lost wake-up)
            if (sleepers_ > 0) cv_.notify_all();
        }
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t spins = 1;; ++spins) {
            if (done_.load(std::memory_order_acquire) == n_) break;
            cpu_relax();
            if ((spins & 0xffu) == 0u &&
                std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > kSpinUs) {
                std::unique_lock<std::mutex> lk(mu_);   // a long job (mirror build, filtered search): sleep until the last worker reports
                done_cv_.wait(lk, [&] { return done_.load(std::memory_order_acquire) == n_; });
                break;
            }
        }
        job_.store(nullptr, std::memory_order_release);
    }

  public:
    void stop() {
        {
            std::unique_lock<std::mutex> lk(mu_);
            stop_.store(true);
            cv_.notify_all();
        }
        for (auto& t : threads_) t.join();
        threads_.clear();
    }

  private:
    std::mutex mu_, job_mu_;
    std::condition_variable cv_, done_cv_;
    std::vector<std::thread> threads_;
    std::atomic<const std::function<void(size_t)>*> job_{nullptr};
    std::atomic<uint64_t> epoch_{0};
    std::atomic<size_t> done_{0};
    std::atomic<bool> stop_{false};
    size_t n_ = 0;
    int sleepers_ = 0;                               // guarded by mu_
};
