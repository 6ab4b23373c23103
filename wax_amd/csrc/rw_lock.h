// rw_lock.h — the engine's reader/writer lock and the count of uncollected tickets per submitting thread. Plain C++17 over the
// standard library: no HIP and no project header; tests/rw_lock/driver.cpp runs the re-entrancy rule and the hand-over of a ticket to
// another thread on the CPU.
#pragma once

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <map>
#include <mutex>
#include <thread>

// Writer-preferring reader/writer lock with thread-agnostic unlock (a ticket may be
// collected on another thread). Same contract as AsyncReadWriteLock
// (WaxCore/Concurrency/ReadWriteLock.swift:79-156).
class RWLock {
  public:
    // reentrant = the caller already holds a shared lock (an uncollected search ticket): it must not queue
    // behind a waiting writer, or the writer (waiting for readers == 0) and the reader (waiting for the
    // writer) deadlock. With readers_ > 0 no writer can be active, so skipping the preference is safe.
    void lock_shared(bool reentrant = false) {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [&] { return !writer_ && (reentrant || writers_waiting_ == 0); });
        ++readers_;
    }
    void unlock_shared() {
        std::unique_lock<std::mutex> g(m_);
        if (--readers_ == 0) cv_.notify_all();
    }
    void lock() {
        std::unique_lock<std::mutex> g(m_);
        ++writers_waiting_;
        cv_.wait(g, [&] { return !writer_ && readers_ == 0; });
        --writers_waiting_;
        writer_ = true;
        epoch_.fetch_add(1, std::memory_order_relaxed);   // every writer: what is cached per store state (the predicate tickets' bitmaps) is of an older epoch now
    }
    // the number of exclusive acquisitions so far: constant while a shared lock is held
    uint64_t epoch() const { return epoch_.load(std::memory_order_relaxed); }
    void unlock() {
        std::unique_lock<std::mutex> g(m_);
        writer_ = false;
        cv_.notify_all();
    }

  private:
    std::mutex m_;
    std::condition_variable cv_;
    int readers_ = 0;
    int writers_waiting_ = 0;
    bool writer_ = false;
    std::atomic<uint64_t> epoch_{0};
};

struct WriteGuard {
    RWLock& l;
    explicit WriteGuard(RWLock& l_) : l(l_) { l.lock(); }
    ~WriteGuard() { l.unlock(); }
};

// Uncollected search tickets per SUBMITTING thread (a ticket holds the shared lock until it is collected, possibly
// by another thread): lets a thread that already holds the lock re-enter past a queued writer, never wait for a
// workspace (work_pool.h), and be refused by the mutating entry points instead of dead-locking on itself.
class TicketHolders {
  public:
    void note_submit(std::thread::id* owner) {
        *owner = std::this_thread::get_id();
        std::unique_lock<std::mutex> g(mu_);
        outstanding_[*owner] += 1;
    }
    void note_collect(std::thread::id owner) {
        std::unique_lock<std::mutex> g(mu_);
        auto it = outstanding_.find(owner);
        if (it != outstanding_.end() && --it->second <= 0) outstanding_.erase(it);
    }
    int holding() const {   // uncollected tickets submitted by the calling thread
        std::unique_lock<std::mutex> g(mu_);
        auto it = outstanding_.find(std::this_thread::get_id());
        return it == outstanding_.end() ? 0 : it->second;
    }

  private:
    mutable std::mutex mu_;
    std::map<std::thread::id, int> outstanding_;
};
