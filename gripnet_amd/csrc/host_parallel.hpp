// What every plan builder's host side runs on: the builder threads (parallel_for over fixed chunks), the host arena the
// builders' large arrays come out of, and the stage timer.  No HIP in here, so that the layout headers on top of it also
// build with plain g++ (tests/host_layout_san.cpp runs them under the sanitizers).
#pragma once

#include <algorithm>
#include <atomic>
#include <condition_variable>
#ifdef GN_LAYOUT_TIMES
#include <chrono>
#include <cstdio>
#endif
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include <unistd.h>

namespace gn {

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The builder threads: parked between builds (a plan of pose0-syn runs thirty parallel passes of a fraction of a
// millisecond each, and starting fifteen threads for every pass was 0.3-0.5 ms of it - a quarter of the decoder plan's build
// time).  One pass at a time uses the pool (a second builder, or a pass started from inside a pass, starts its own threads
// as before); the pool belongs to the process that made it - after a fork the child makes its own at its first pass (the
// parent's threads do not exist there) - and is never torn down.
struct WorkerPool {
    std::mutex run_lock;               // held by the pass that is using the pool
    std::mutex m;                      // guards everything below
    std::condition_variable wake, done;
    std::vector<std::thread> threads;
    std::function<void(int64_t)> job;  // job(chunk)
    int64_t chunks = 0, next = 0, pending = 0;
    uint64_t generation = 0;
    long owner = 0;                    // the process the threads live in
};
inline void pool_worker(WorkerPool* p, uint64_t seen) {
    std::unique_lock<std::mutex> lk(p->m);
    for (;;) {
        p->wake.wait(lk, [&] { return p->generation != seen; });
        seen = p->generation;
        while (p->next < p->chunks) {
            const int64_t c = p->next++;
            lk.unlock();
            p->job(c);
            lk.lock();
            if (--p->pending == 0) p->done.notify_one();
        }
    }
}
inline WorkerPool* worker_pool() {
    static std::atomic<WorkerPool*> pool{nullptr};
    WorkerPool* p = pool.load(std::memory_order_acquire);
    const long me = (long)getpid();
    if (p != nullptr && p->owner == me) return p;
    WorkerPool* fresh = new WorkerPool();                     // (a pool inherited through fork is left alone: its threads are gone)
    fresh->owner = me;
    if (pool.compare_exchange_strong(p, fresh, std::memory_order_acq_rel)) return fresh;
    delete fresh;
    p = pool.load(std::memory_order_acquire);
    return (p != nullptr && p->owner == me) ? p : nullptr;
}

// Host side of the plan builders: fn(begin, end) over contiguous chunks of [0, n) on up to GN_PLAN_THREADS (default 16:
// the CPU share of one GPU on the boxes this runs on) threads.  The chunks are fixed by n and the thread count only and
// every chunk writes its own outputs, so a plan does not depend on scheduling.
template <typename F>
inline void parallel_for(int64_t n, int64_t grain, F fn) {
    int want = 16;
    if (const char* e = getenv("GN_PLAN_THREADS")) want = std::max(1, atoi(e));
    const unsigned hw = std::thread::hardware_concurrency();
    if (hw > 0) want = std::min<int>(want, (int)hw);
    const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>(want, (n + grain - 1) / std::max<int64_t>(grain, 1)));
    if (chunks <= 1 || n <= 0) { if (n > 0) fn((int64_t)0, n); return; }
    WorkerPool* p = worker_pool();
    if (p != nullptr && p->run_lock.try_lock()) {
        std::unique_lock<std::mutex> lk(p->m);
        while ((int64_t)p->threads.size() < chunks - 1) p->threads.emplace_back(pool_worker, p, p->generation);
        p->job = [&](int64_t c) { fn(n * c / chunks, n * (c + 1) / chunks); };
        p->chunks = chunks; p->next = 1; p->pending = chunks - 1;
        ++p->generation;
        lk.unlock();
        p->wake.notify_all();
        fn((int64_t)0, n / chunks);
        lk.lock();
        while (p->next < p->chunks) {                          // (chunks no parked thread has picked up yet)
            const int64_t c = p->next++;
            lk.unlock();
            fn(n * c / chunks, n * (c + 1) / chunks);
            lk.lock();
            --p->pending;
        }
        p->done.wait(lk, [&] { return p->pending == 0; });
        p->job = nullptr;
        p->chunks = 0; p->next = 0;
        lk.unlock();
        p->run_lock.unlock();
        return;
    }
    std::vector<std::thread> pool;
    pool.reserve((size_t)chunks - 1);
    for (int64_t c = 1; c < chunks; ++c) pool.emplace_back([=]() { fn(n * c / chunks, n * (c + 1) / chunks); });
    fn((int64_t)0, n / chunks);
    for (std::thread& t : pool) t.join();
}

// The builders' large host arrays come out of ONE block of the process that is kept between builds (grow-only up to
// kMaxBytes, never given back).  A plan of pose0-syn asks for ~90 MB in arrays of 2-16 MB; malloc serves each with a fresh
// mapping and free unmaps it, and in a long-lived process (bench.py after its training epochs) that traffic with the kernel
// - page faults on every first touch, the unmapping at the end - cost as much as the builders' own work: decoder plan 17 ms of
// builders, 27-32 ms measured; 17.8 ms with glibc told to keep its heap (MALLOC_MMAP_THRESHOLD_ / MALLOC_TRIM_THRESHOLD_).
// A builder takes the arena for its scope (ArenaHold, FIRST local of the entry point: every array dies before it); arrays
// of at least kMinBytes are bump-allocated from it on the holder's thread, everything else - and everything while another
// builder holds the arena, and what does not fit - is plain malloc.  The block grows to 5/4 of what the last holder asked
// for, at the next acquire.  No array may outlive its hold.
struct HostArena {
    static constexpr size_t kMaxBytes = (size_t)1 << 30;
    static constexpr size_t kMinBytes = (size_t)256 << 10;
    std::mutex lock;
    std::atomic<char*> base{nullptr};  // (read by arena_owns on any thread, without the lock: see the order of the stores in ArenaHold)
    std::atomic<size_t> bytes{0};
    size_t want = 0;                   // what the block should hold at the next acquire
    std::atomic<size_t> used{0};       // bump pointer of the current hold
    std::atomic<size_t> asked{0};      // bytes requested during the current hold (served or not)
};
inline HostArena& host_arena() {
    static HostArena arena;
    return arena;
}
inline HostArena*& arena_of_this_thread() {
    static thread_local HostArena* held = nullptr;
    return held;
}
struct ArenaHold {
    bool held = false;
    ArenaHold() {
        HostArena& a = host_arena();
        if (arena_of_this_thread() != nullptr || !a.lock.try_lock()) return;     // (nested, or another builder has it: malloc)
        held = true;
        if (a.want > a.bytes.load()) {
            // a thread without the arena may be asking arena_owns() about a pointer of its own right now: it reads `bytes`, then
            // `base` - the size goes to zero before the block changes and comes back after it, so that no mix of old and new spans
            // memory that is not the block's
            char* old = a.base.load();
            a.bytes.store(0);
            a.base.store(nullptr);
            std::free(old);
            char* fresh = static_cast<char*>(std::malloc(a.want));
            a.base.store(fresh);
            a.bytes.store(fresh ? a.want : 0);
        }
        a.used.store(0); a.asked.store(0);
        arena_of_this_thread() = &a;
    }
    ArenaHold(const ArenaHold&) = delete;
    ArenaHold& operator=(const ArenaHold&) = delete;
    ~ArenaHold() {
        if (!held) return;
        HostArena& a = host_arena();
        arena_of_this_thread() = nullptr;
        const size_t asked = a.asked.load();
        a.want = std::max(a.want, std::min(HostArena::kMaxBytes, asked + asked / 4));
        a.lock.unlock();
    }
};
inline void* arena_allocate(size_t bytes) {
    HostArena* a = arena_of_this_thread();
    if (a == nullptr || bytes < HostArena::kMinBytes) return nullptr;
    const size_t padded = (bytes + 63) & ~(size_t)63;
    a->asked.fetch_add(padded);
    const size_t at = a->used.fetch_add(padded);
    if (at + padded > a->bytes.load()) { a->used.fetch_sub(padded); return nullptr; }
    return a->base.load() + at;
}
inline bool arena_owns(const void* p) {
    const HostArena& a = host_arena();
    const size_t bytes = a.bytes.load();
    const char* base = a.base.load();
    return base != nullptr && static_cast<const char*>(p) >= base && static_cast<const char*>(p) < base + bytes;
}

// A vector whose resize() leaves new elements uninitialised (the builders' large arrays are written whole by the parallel
// passes that follow: a value-initialising resize was a serial walk - and the first touch - of every page), and whose large
// blocks come from the arena above while the calling thread holds it.
template <typename T>
struct DefaultInit : std::allocator<T> {
    template <typename U> struct rebind { using other = DefaultInit<U>; };
    template <typename U> void construct(U* ptr) noexcept(std::is_nothrow_default_constructible<U>::value) { ::new (static_cast<void*>(ptr)) U; }
    template <typename U, typename... A> void construct(U* ptr, A&&... a) { ::new (static_cast<void*>(ptr)) U(std::forward<A>(a)...); }
    T* allocate(size_t n) {
        if (void* p = arena_allocate(n * sizeof(T))) return static_cast<T*>(p);
        return std::allocator<T>::allocate(n);
    }
    void deallocate(T* p, size_t n) {
        if (arena_owns(p)) return;                           // (the block is reused whole by the next holder)
        std::allocator<T>::deallocate(p, n);
    }
};
template <typename T>
using RawVec = std::vector<T, DefaultInit<T>>;

// v = n copies of `value`, written (and first touched) by the builder threads
template <typename V, typename T>
inline void parallel_assign(V& v, size_t n, T value) {
    v.resize(n);
    parallel_for((int64_t)n, 1 << 16, [&](int64_t i0, int64_t i1) { std::fill(v.begin() + i0, v.begin() + i1, value); });
}

}  // namespace gn

namespace gn_layout {

// Stage times of the builders on stderr when compiled with -DGN_LAYOUT_TIMES (tools/probes/plan_host_time.cpp); nothing otherwise.
#ifdef GN_LAYOUT_TIMES
inline void lap(const char* what) {
    static thread_local double last = 0.0;
    const double t = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    if (what) std::fprintf(stderr, "    %-34s %7.2f ms\n", what, 1e3 * (t - last));
    last = t;
}
#define GN_LAP(what) gn_layout::lap(what)
#else
#define GN_LAP(what) ((void)0)
#endif

}  // namespace gn_layout
