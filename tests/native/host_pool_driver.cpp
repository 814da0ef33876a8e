// Driver for csrc/p2s_host.h (tests/test_host_pool.py), built with -fsanitize=address,undefined: the pool visits every
// index once, survives a body that runs out of memory, and the thread-count rule and the UTF-8 check answer as stated.
#include <atomic>
#include <cstdio>
#include <memory>

#include "p2s_host.h"

static int failures = 0;
#define CHECK(cond, ...) \
    do { if (!(cond)) { ++failures; fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

// One ordinary call: true, every index of [0, n) exactly once, thread within [0, n_threads), no empty chunk but for n = 0.
static void check_coverage(int64_t n, int64_t grain, int n_threads) {
    std::unique_ptr<std::atomic<int>[]> seen(new std::atomic<int>[(size_t)n + 1]);
    for (int64_t i = 0; i <= n; ++i) seen[(size_t)i] = 0;
    std::atomic<int> calls{0}, bad_thread{0}, bad_range{0};
    const bool ok = parallel_for(n, n_threads, grain, [&](int t, int64_t lo, int64_t hi) {
        ++calls;
        if (t < 0 || t >= n_threads) ++bad_thread;
        if (lo < 0 || hi > n || lo > hi || (lo == hi && n > 0) || hi - lo > grain) { ++bad_range; return; }
        for (int64_t i = lo; i < hi; ++i) ++seen[(size_t)i];
    });
    int64_t wrong = 0;
    for (int64_t i = 0; i < n; ++i) wrong += seen[(size_t)i] != 1;
    CHECK(ok, "n=%lld grain=%lld threads=%d", (long long)n, (long long)grain, n_threads);
    CHECK(wrong == 0 && seen[(size_t)n] == 0, "n=%lld grain=%lld threads=%d: %lld indices not visited once", (long long)n, (long long)grain, n_threads, (long long)wrong);
    CHECK(bad_thread == 0 && bad_range == 0, "n=%lld grain=%lld threads=%d: %d thread numbers, %d ranges out of bounds", (long long)n, (long long)grain, n_threads, bad_thread.load(), bad_range.load());
    if (n == 0) CHECK(calls <= 1, "n=0: %d calls", calls.load());
}

static void check_throwing_body(int n_threads) {
    const bool ok = parallel_for(100000, n_threads, 64, [&](int, int64_t lo, int64_t) {
        if (lo == 128) throw std::bad_alloc();
    });
    CHECK(!ok, "threads=%d: a body that threw std::bad_alloc must make the call return false", n_threads);
    check_coverage(100000, 64, n_threads);                    // the process goes on, and so does the pool
}

int main() {
    for (int64_t n : {0, 1, 63, 64, 65, 1000})
        for (int64_t grain : {1, 64, 4096})
            for (int n_threads : {1, 2, 8}) check_coverage(n, grain, n_threads);
    check_throwing_body(8);
    check_throwing_body(1);

    const int any = host_threads(0, 16, 1000000);
    CHECK(any >= 1 && any <= 16, "host_threads(0, 16, 1e6) = %d", any);
    CHECK(host_threads(5, 16, 3) == 3, "got %d", host_threads(5, 16, 3));
    CHECK(host_threads(5, 16, 0) == 1, "got %d", host_threads(5, 16, 0));
    CHECK(host_threads(100, 32, 1000000) == 32, "got %d", host_threads(100, 32, 1000000));

    const struct { const char *bytes; size_t n; bool valid; const char *what; } utf8[] = {
        {"plain ASCII", 11, true, "ASCII"},
        {"\xC3\xA9", 2, true, "2-byte sequence"},
        {"\xE2\x82\xAC", 3, true, "3-byte sequence"},
        {"\xF0\x9F\x98\x80", 4, true, "4-byte sequence"},
        {"\xF4\x8F\xBF\xBF", 4, true, "U+10FFFF"},
        {"\xC0\x80", 2, false, "overlong 2-byte NUL"},
        {"\xED\xA0\x80", 3, false, "surrogate"},
        {"\xF4\x90\x80\x80", 4, false, "beyond U+10FFFF"},
        {"ab\xE2\x82", 4, false, "sequence cut off at the end"},
        {"a\x80z", 3, false, "lone continuation byte"},
    };
    for (const auto &u : utf8)
        CHECK(valid_utf8((const unsigned char *)u.bytes, u.n) == u.valid, "%s", u.what);

    if (failures) return 1;
    puts("host pool ok");
    return 0;
}
