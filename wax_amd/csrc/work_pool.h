// work_pool.h — the pools of per-call workspaces and the ticket tables. Plain C++17 over the standard library: no HIP and no
// project header, so tests/work_pool/driver.cpp runs them on the CPU under sanitizers, single-threaded against a model and with real
// threads.
//
// WorkPool<T> owns every item it ever made (`all`), hands out the idle ones (`free`) and makes a new one while fewer than `cap` exist.
// What acquire() does when `cap` items exist and none is idle is the caller's PoolMode:
//
//   wait   sleep until a release (or a raised cap)        a caller that holds no ticket of the engine
//   tries  PoolGot::busy at once                          a caller that can do something else instead (collect a ticket of its own)
//   grow   make one more, up to the hard cap; then        a thread that already holds tickets: each ticket holds an item of the pool AND
//          PoolGot::exhausted                             the engine's shared lock. Two such threads that each hold half of the pool and
//                                                         wait for one more wait for each other for ever, and every writer behind them —
//                                                         so a holder never waits: it gets a fresh item or a refusal
//
// Which pool uses which: the single-query scratch slots tries / grow / wait (in this order of precedence, 256 the hard cap); the sharded
// single-query slots grow / wait (8, hard cap 64); the batch workspaces, single and sharded, tries / wait; the filtered-search workspaces
// wait only. Items past the soft cap stay pooled.
//
// TicketTable<T> numbers what is in flight: ids from 1, never reused, taken exactly once. It has a mutex of its own: no caller needs a
// pool operation and a ticket operation to happen as one (a submit puts the ticket after it has the item, a collect takes the ticket
// before it releases the item, and `empty()` is a planning figure).
#pragma once

#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

enum class PoolMode { wait, tries, grow };
enum class PoolGot {
    reused,      // an idle item
    fresh,       // made by this call (and registered)
    busy,        // PoolMode::tries: every item is in use
    exhausted,   // PoolMode::grow: every item is in use and the hard cap is reached
    failed,      // `make` failed: its code is in *make_rc, nothing was registered
};

template <typename T>
class WorkPool {
public:
    explicit WorkPool(int cap, int hard_cap = 0) : cap_(cap), hard_cap_(hard_cap) {}
    WorkPool(const WorkPool&) = delete;
    WorkPool& operator=(const WorkPool&) = delete;

    // make(index, T** out) -> 0 or an error code; it runs under the pool's lock, so the cap check and the registration are one step, and
    // `index` is the item's position in `all` for good. Nothing is allocated on the way to an idle item.
    template <typename Make>
    PoolGot acquire(PoolMode mode, T** out, int* make_rc, Make&& make) {
        std::unique_lock<std::mutex> g(mu_);
        for (;;) {
            if (!free_.empty()) {
                *out = free_.back();
                free_.pop_back();
                return PoolGot::reused;
            }
            const int n = (int)all_.size();
            if (n < cap_ || (mode == PoolMode::grow && n < hard_cap_)) {
                T* item = nullptr;
                *make_rc = make(n, &item);
                if (*make_rc != 0) return PoolGot::failed;
                all_.push_back(item);
                *out = item;
                return PoolGot::fresh;
            }
            if (mode == PoolMode::tries) return PoolGot::busy;
            if (mode == PoolMode::grow) return PoolGot::exhausted;
            cv_.wait(g);
        }
    }
    void release(T* item) {
        std::unique_lock<std::mutex> g(mu_);
        free_.push_back(item);
        cv_.notify_one();
    }
    // an item made outside acquire() (the one created with the engine): registered and idle
    void seed(T* item) {
        std::unique_lock<std::mutex> g(mu_);
        all_.push_back(item);
        free_.push_back(item);
    }
    // A lowered cap takes nothing away: the items that exist stay pooled and are reused. A raised one wakes the waiters, who may now make one.
    void set_cap(int cap) {
        std::unique_lock<std::mutex> g(mu_);
        cap_ = cap;
        cv_.notify_all();
    }
    int cap() const {
        std::unique_lock<std::mutex> g(mu_);
        return cap_;
    }
    size_t size() const {
        std::unique_lock<std::mutex> g(mu_);
        return all_.size();
    }
    // fn(T*) on every item, idle or in use, under the pool's lock
    template <typename Fn>
    void for_each(Fn&& fn) const {
        std::unique_lock<std::mutex> g(mu_);
        for (T* item : all_) fn(item);
    }
    // destroy: fn(T*) frees every item; the pool is empty afterwards (no item may be in use)
    template <typename Fn>
    void drain(Fn&& fn) {
        std::unique_lock<std::mutex> g(mu_);
        for (T* item : all_) fn(item);
        all_.clear();
        free_.clear();
    }

private:
    mutable std::mutex mu_;
    std::condition_variable cv_;
    std::vector<T*> all_, free_;
    int cap_;
    const int hard_cap_;   // 0: PoolMode::grow is never asked for
};

template <typename T>
class TicketTable {
public:
    uint64_t put(T v) {
        std::unique_lock<std::mutex> g(mu_);
        const uint64_t id = next_++;
        map_.emplace(id, std::move(v));
        return id;
    }
    // false: an unknown id (never given out, or taken already)
    bool take(uint64_t id, T* out) {
        std::unique_lock<std::mutex> g(mu_);
        auto it = map_.find(id);
        if (it == map_.end()) return false;
        *out = std::move(it->second);
        map_.erase(it);
        return true;
    }
    // fn(const T&) under the table's lock, the ticket stays
    template <typename Fn>
    bool peek(uint64_t id, Fn&& fn) const {
        std::unique_lock<std::mutex> g(mu_);
        auto it = map_.find(id);
        if (it == map_.end()) return false;
        fn(it->second);
        return true;
    }
    bool empty() const {
        std::unique_lock<std::mutex> g(mu_);
        return map_.empty();
    }

private:
    mutable std::mutex mu_;
    std::map<uint64_t, T> map_;
    uint64_t next_ = 1;
};
