// Sanitizer driver for the host code of the primary-person extraction (tests/test_extract_sanitized.py): parses every file
// named on stdin, gathers the per-person flags, and writes single-person documents of the three kinds -- extreme floats,
// integers up to the ends of int64 -- plus the calls the writer must refuse, under -fsanitize=address,undefined.
// usage: extract_driver THREADS OUTPUT_FOLDER < paths
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "p2s.h"

int p2s_set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    return code;
}

int main(int argc, char **argv) {
    if (argc < 3) return 1;
    const int threads = atoi(argv[1]);
    const std::string folder = argv[2];
    std::string blob, line;
    std::vector<int64_t> off{0};
    while (std::getline(std::cin, line)) {
        blob += line;
        off.push_back((int64_t)blob.size());
    }
    const int64_t n = (int64_t)off.size() - 1;
    p2s_json_batch *b = nullptr;
    if (p2s_json_parse(blob.data(), off.data(), n, threads, &b) != P2S_OK) return 2;
    std::vector<int64_t> base((size_t)n + 1);
    if (p2s_json_people_counts(b, nullptr, base.data()) != P2S_OK) return 3;
    std::vector<int32_t> flags((size_t)base[(size_t)n] + 1, -1);
    if (p2s_json_person_flags(b, flags.data()) != P2S_OK) return 4;
    int64_t ints = 0;
    for (int64_t i = 0; i < base[(size_t)n]; ++i) {
        if (flags[(size_t)i] < 0 || flags[(size_t)i] > 63) return 5;
        ints += flags[(size_t)i] & P2S_JSON_PERSON_ALL_INTS;
    }
    if (flags.back() != -1) return 6;                                  // nothing beyond the last person is written
    if (p2s_json_person_flags(b, nullptr) == P2S_OK || p2s_json_person_flags(nullptr, flags.data()) == P2S_OK) return 7;
    p2s_json_free(b);

    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double odd[] = {0.0, -0.0, 1e22, 1e21, 1e16, 5e-324, 1.7976931348623157e308, -2.2250738585072014e-308, 0.1, 1.0 / 3, nan, inf, -inf, 123456789.12345678};
    const double whole[] = {0.0, -1.0, 9007199254740992.0, -9223372036854775808.0, 9223372036854774784.0, 10000000000.0};
    for (int n_kpts : {1, 26, 127}) {
        const int64_t files = 300, nv = 3 * n_kpts;
        std::vector<double> values((size_t)(files * nv));
        std::vector<int8_t> kind((size_t)files), written((size_t)files + 1, 7);
        std::string paths;
        std::vector<int64_t> po{0};
        for (int64_t i = 0; i < files; ++i) {
            kind[(size_t)i] = (int8_t)(i % 3);
            for (int64_t k = 0; k < nv; ++k)
                values[(size_t)(i * nv + k)] = kind[(size_t)i] == 2 ? whole[(i + k) % 6] : odd[(i * 7 + k) % 14] * (1 + (double)k);
            paths += i % 50 == 49 ? folder + "/missing/x.json" : folder + "/k" + std::to_string(n_kpts) + "_" + std::to_string(i) + ".json";
            po.push_back((int64_t)paths.size());
        }
        if (p2s_write_person_files(paths.data(), po.data(), files, values.data(), kind.data(), n_kpts, threads, written.data()) != P2S_OK) return 8;
        for (int64_t i = 0; i < files; ++i)
            if (written[(size_t)i] != (i % 50 == 49 ? 0 : 1)) return 9;
        if (written.back() != 7) return 10;
        values[(size_t)(2 * nv)] = 0.5;                                 // file 2 is of kind 2: not an integer
        if (p2s_write_person_files(paths.data(), po.data(), files, values.data(), kind.data(), n_kpts, threads, nullptr) == P2S_OK) return 11;
        values[(size_t)(2 * nv)] = 9223372036854775808.0;               // 2^63: beyond int64
        if (p2s_write_person_files(paths.data(), po.data(), files, values.data(), kind.data(), n_kpts, threads, nullptr) == P2S_OK) return 12;
        values[(size_t)(2 * nv)] = nan;
        if (p2s_write_person_files(paths.data(), po.data(), files, values.data(), kind.data(), n_kpts, threads, nullptr) == P2S_OK) return 13;
        kind[0] = 3;
        if (p2s_write_person_files(paths.data(), po.data(), files, values.data(), kind.data(), n_kpts, threads, nullptr) == P2S_OK) return 14;
    }
    if (p2s_write_person_files(nullptr, nullptr, 0, nullptr, nullptr, 26, threads, nullptr) != P2S_OK) return 15;
    if (p2s_write_person_files(nullptr, nullptr, 0, nullptr, nullptr, 128, threads, nullptr) == P2S_OK) return 16;
    printf("files %lld persons %lld all-integer %lld\n", (long long)n, (long long)base[(size_t)n], (long long)ints);
    return 0;
}
