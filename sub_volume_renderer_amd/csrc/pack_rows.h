// The host half of an upload: the gather of a strided host block into a packed staging buffer, dealt to a few kept
// threads.  Plain host C++ on plain bytes, so that a test can compile it without HIP (tests/test_pack_rows.py);
// svr_upload.hip packs every staged block of svr_upload_region with it.
#pragma once

#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

// Copy rows [r0, r1) of a strided host block into a packed buffer (x fastest); a row index is z * shape[1] + y.
static inline void pack_row_range(const char* src, size_t es, const int64_t st[3], const int32_t shape[3],
                                  int64_t r0, int64_t r1, char* dst) {
    const size_t row = (size_t)shape[0] * es;
    for (int64_t r = r0; r < r1; ++r) {
        const int64_t z = r / shape[1], y = r % shape[1];
        const char* s = src + z * st[2] + y * st[1];
        if (st[0] == (int64_t)es) memcpy(dst, s, row);
        else for (int x = 0; x < shape[0]; ++x) memcpy(dst + (size_t)x * es, s + (int64_t)x * st[0], es);
        dst += row;
    }
}

// The host half of an upload is a gather of short rows (48 .. 528 voxels) out of a large strided array into the
// pinned staging slot: one core moves ~6-15 GB/s that way, well under the PCIe rate, so the rows are dealt to a
// few threads (contiguous row ranges).  The threads are kept: a block is a few MiB to tens of MiB, i.e. 0.1-1 ms
// of copying, and starting 7 threads per block costs a good part of that.
class PackPool {
public:
    static PackPool& get() {
        static std::mutex mu;
        static PackPool* pool = nullptr;
        static pid_t owner = 0;
        std::lock_guard<std::mutex> g(mu);
        if (!pool || owner != getpid()) { pool = new PackPool(); owner = getpid(); }   // threads do not survive fork(): the child starts its own (the parent's object is left alone)
        return *pool;
    }
    static constexpr int kMax = 16;
    // fn(t) for t in [0, nt): t = 0 on the caller, the rest on the workers; returns when all are done
    void run(int nt, const std::function<void(int)>& fn) {
        nt = std::min(nt, kMax);
        if (nt <= 1) { fn(0); return; }
        std::lock_guard<std::mutex> one(run_mu);
        {
            std::lock_guard<std::mutex> g(mu);
            while ((int)workers.size() < nt - 1) { const int id = (int)workers.size() + 1; workers.emplace_back([this, id] { loop(id); }); }
            job = &fn; want = nt; left = nt - 1; ++gen;
        }
        go.notify_all();
        fn(0);
        std::unique_lock<std::mutex> g(mu);
        done.wait(g, [this] { return left == 0; });
        job = nullptr;
    }
    ~PackPool() {
        { std::lock_guard<std::mutex> g(mu); stop = true; }
        go.notify_all();
        for (auto& w : workers) w.join();
    }
private:
    void loop(int id) {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> g(mu);
        for (;;) {
            go.wait(g, [&] { return stop || gen != seen; });
            if (stop) return;
            seen = gen;
            if (id >= want) continue;
            const std::function<void(int)>* f = job;
            g.unlock();
            (*f)(id);
            g.lock();
            if (--left == 0) done.notify_one();
        }
    }
    std::vector<std::thread> workers;
    std::mutex mu, run_mu;
    std::condition_variable go, done;
    const std::function<void(int)>* job = nullptr;
    uint64_t gen = 0;
    int want = 0, left = 0;
    bool stop = false;
};

// Pack rows [r0, r1) of the density block and of the label block (either may be absent) in one parallel pass.
static inline void pack_rows(const char* dsrc, size_t des, const int64_t* dst_strides, char* ddst,
                             const char* lsrc, size_t les, const int64_t* lst_strides, char* ldst,
                             const int32_t shape[3], int64_t r0, int64_t r1) {
    const int64_t nrows = r1 - r0;
    const size_t bytes = (size_t)shape[0] * (size_t)nrows * ((dsrc ? des : 0) + (lsrc ? les : 0));
    unsigned hw = std::thread::hardware_concurrency();
    // (12 or 16 threads, and streaming stores into the slot, measured no faster)
    int nt = (int)std::min<size_t>(std::min<unsigned>(hw ? hw : 1u, 8u), bytes / ((size_t)512 << 10));
    if (const char* e = getenv("SVR_PACK_THREADS")) nt = std::max(1, atoi(e));      // deployment setting (include/svr.h), not an experiment
    nt = (int)std::min<int64_t>(std::max(nt, 1), std::max<int64_t>(1, nrows / 2));
    const int64_t per = (nrows + nt - 1) / nt;
    PackPool::get().run(nt, [&](int t) {
        const int64_t a = r0 + per * t, b = std::min(r1, a + per);
        if (a >= b) return;
        if (dsrc) pack_row_range(dsrc, des, dst_strides, shape, a, b, ddst + (size_t)(a - r0) * shape[0] * des);
        if (lsrc) pack_row_range(lsrc, les, lst_strides, shape, a, b, ldst + (size_t)(a - r0) * shape[0] * les);
    });
}
