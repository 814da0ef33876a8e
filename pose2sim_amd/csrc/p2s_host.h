// p2s_host.h -- what the host-only translation units (p2s_ingest.cpp, p2s_rewrite.cpp, p2s_trc.cpp, p2s_proposals.cpp)
// share: the one thread pool, the thread-count rule, the strict UTF-8 check and the read-a-whole-file loop.  Standard
// library and POSIX only, no HIP.
#ifndef P2S_HOST_H
#define P2S_HOST_H

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <unistd.h>

namespace {

// Host threads for `tasks` pieces of work: the count asked for, else the machine's; at least 1, at most `cap`, and no
// more than there are tasks.
inline int host_threads(int32_t asked, int cap, int64_t tasks) {
    int n = asked > 0 ? asked : (int)std::thread::hardware_concurrency();
    if (n < 1) n = 1;
    if (n > cap) n = cap;
    if ((int64_t)n > tasks) n = (int)(tasks > 0 ? tasks : 1);
    return n;
}

// fn(thread, lo, hi) over [0, n) in chunks of `grain` indices handed out by one counter; thread in [0, n_threads).  The
// caller is worker 0 and n_threads - 1 threads run beside it.  A std::bad_alloc from fn (the only exception a body may
// throw) is caught on the worker it was thrown on: no further chunk is handed out, every thread is joined, the result
// is false.  A thread that cannot be started is no error: the ones that did start, and the caller, do the work.
template <typename Fn>
bool parallel_for(int64_t n, int n_threads, int64_t grain, Fn fn) {
    std::atomic<int64_t> next{0};
    std::atomic<bool> failed{false};
    auto work = [&](int t) {
        try {
            while (!failed.load(std::memory_order_relaxed)) {
                const int64_t lo = next.fetch_add(grain);
                if (lo >= n) break;
                fn(t, lo, lo + grain < n ? lo + grain : n);
            }
        } catch (const std::bad_alloc &) {
            failed.store(true);
        }
    };
    std::vector<std::thread> pool;
    try {
        if (n_threads > 1) pool.reserve((size_t)n_threads - 1);
        for (int t = 1; t < n_threads; ++t) pool.emplace_back(work, t);
    } catch (const std::system_error &) {                     // EAGAIN: go on with the threads there are
    } catch (const std::bad_alloc &) {
    }
    work(0);
    for (auto &th : pool) th.join();
    return !failed.load();
}

// Strict UTF-8 (what open(path, 'r') decodes with): no overlongs, no surrogates, <= U+10FFFF.
inline bool valid_utf8(const unsigned char *s, size_t n) {
    size_t i = 0;
    while (i < n) {
        const unsigned char c = s[i];
        if (c < 0x80) {
            ++i;
            continue;
        }
        int len;
        uint32_t cp;
        if ((c & 0xE0) == 0xC0) { len = 2; cp = c & 0x1F; }
        else if ((c & 0xF0) == 0xE0) { len = 3; cp = c & 0x0F; }
        else if ((c & 0xF8) == 0xF0) { len = 4; cp = c & 0x07; }
        else return false;
        if (i + len > n) return false;
        for (int k = 1; k < len; ++k) {
            if ((s[i + k] & 0xC0) != 0x80) return false;
            cp = (cp << 6) | (s[i + k] & 0x3F);
        }
        if ((len == 2 && cp < 0x80) || (len == 3 && cp < 0x800) || (len == 4 && cp < 0x10000)) return false;
        if (cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF)) return false;
        i += len;
    }
    return true;
}

// The whole file into buf (grown as needed, never shrunk); n = its size.  false when it cannot be opened or read.
inline bool read_file(const char *path, std::vector<char> &buf, size_t &n) {
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return false;
    struct Closer { int fd; ~Closer() { close(fd); } } closer{fd};   // also when resize throws
    n = 0;
    if (buf.size() < 16384) buf.resize(16384);
    while (true) {
        if (n == buf.size()) buf.resize(buf.size() * 2);
        const ssize_t r = read(fd, buf.data() + n, buf.size() - n);
        if (r < 0) return false;
        if (r == 0) return true;
        n += (size_t)r;
    }
}

}  // namespace

#endif
