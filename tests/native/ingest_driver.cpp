// Sanitizer driver for the host-only translation units (tests/test_ingest_sanitized.py): parses every file named on
// stdin through the public entry points and walks all results, then rewrites and copies the files, writes .trc rows and
// OpenPose files and extracts proposals, under -fsanitize=address,undefined.
// usage: ingest_driver THREADS [TRC_FILE [CAMERA_FOLDER_1 CAMERA_FOLDER_2]] < paths
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
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
    const int threads = argc > 1 ? atoi(argv[1]) : 4;
    std::string blob, line;
    std::vector<int64_t> off{0};
    while (std::getline(std::cin, line)) {
        blob += line;
        off.push_back((int64_t)blob.size());
    }
    const int64_t n = (int64_t)off.size() - 1;
    p2s_json_batch *b = nullptr;
    if (p2s_json_parse(blob.data(), off.data(), n, threads, &b) != P2S_OK) return 2;
    std::vector<int32_t> counts((size_t)n);
    std::vector<int64_t> base((size_t)n + 1);
    if (p2s_json_people_counts(b, counts.data(), base.data()) != P2S_OK) return 3;
    std::vector<int32_t> lens((size_t)base[(size_t)n] + 1);
    if (p2s_json_person_lengths(b, lens.data()) != P2S_OK) return 4;
    const int32_t ids[5] = {0, 3, 1, 25, 1000};
    const int32_t maxp = 3;
    std::vector<int64_t> fo((size_t)n);
    for (int64_t i = 0; i < n; ++i) fo[(size_t)i] = i * maxp * 15;
    std::vector<float> out32((size_t)n * maxp * 15 + 1);
    std::vector<double> out64((size_t)n * maxp * 15 + 1);
    int64_t bad = 0;
    if (p2s_json_gather_keypoints(b, ids, 5, maxp, fo.data(), 15, P2S_F32, out32.data(), &bad) != P2S_OK) return 5;
    if (p2s_json_gather_keypoints(b, ids, 5, maxp, fo.data(), 15, P2S_F64, out64.data(), nullptr) != P2S_OK) return 6;
    std::vector<int64_t> fi;
    std::vector<int32_t> pi;
    for (int64_t i = 0; i < n; ++i)
        for (int32_t p = 0; p < counts[(size_t)i]; ++p) {
            fi.push_back(i);
            pi.push_back(p);
        }
    std::vector<double> rows(fi.size() * 9 + 1);
    if (p2s_json_gather_people(b, fi.data(), pi.data(), (int64_t)fi.size(), 9, P2S_F64, rows.data(), &bad) != P2S_OK) return 7;
    std::vector<double> big((size_t)n * 15 + 1);
    if (p2s_json_gather_largest_person(b, ids, 5, 0.3, big.data()) != P2S_OK) return 10;
    std::vector<int32_t> status((size_t)n + 1), detail((size_t)n + 1);
    if (p2s_json_select_tracked_person(b, 5, 0.3, big.data(), status.data(), detail.data()) != P2S_OK) return 11;
    {
        std::vector<int64_t> text_off((size_t)base[(size_t)n] + 1);
        std::vector<int32_t> kind((size_t)n + 1);
        if (p2s_json_person_ids(b, text_off.data(), nullptr, 0, kind.data()) != P2S_OK) return 12;
        std::vector<char> text((size_t)text_off.back() + 1);
        if (p2s_json_person_ids(b, text_off.data(), text.data(), text_off.back(), kind.data()) != P2S_OK) return 13;
    }
    // rewrite every file with the selection (person 0, {}, person 1, person 2) into <path>.out
    {
        std::string dblob;
        std::vector<int64_t> doff{0}, soff{0};
        std::vector<int32_t> sel;
        for (int64_t i = 0; i < n; ++i) {
            dblob.append(blob, (size_t)off[(size_t)i], (size_t)(off[(size_t)i + 1] - off[(size_t)i]));
            if (off[(size_t)i + 1] > off[(size_t)i]) dblob += ".out";
            doff.push_back((int64_t)dblob.size());
            const int32_t pick[4] = {0, -1, 1, 2};
            for (int k = 0; k < (int)(i % 5); ++k) sel.push_back(pick[k % 4]);
            soff.push_back((int64_t)sel.size());
        }
        std::vector<int8_t> written((size_t)n + 1);
        if (p2s_json_rewrite_people(blob.data(), off.data(), dblob.data(), doff.data(), n, soff.data(), sel.data(), threads,
                                    written.data()) != P2S_OK) return 8;
        // ... and copy it to <path>.copy: a source that cannot be read is reported (P2S_ERR_INVALID_ARG), nothing worse
        std::string cblob;
        std::vector<int64_t> coff{0};
        for (int64_t i = 0; i < n; ++i) {
            cblob.append(blob, (size_t)off[(size_t)i], (size_t)(off[(size_t)i + 1] - off[(size_t)i]));
            if (off[(size_t)i + 1] > off[(size_t)i]) cblob += ".copy";
            coff.push_back((int64_t)cblob.size());
        }
        const int rc = p2s_copy_files(blob.data(), off.data(), cblob.data(), coff.data(), n, threads, written.data());
        if (rc != P2S_OK && rc != P2S_ERR_INVALID_ARG) return 14;
        char tmp[64];
        p2s_format_float_repr(0.1, tmp, 64);
        const char *trc = argc > 2 ? argv[2] : nullptr;
        if (trc) {
            std::vector<int64_t> fr(100);
            std::vector<double> tm(100), dat(100 * 7);
            for (int r = 0; r < 100; ++r) { fr[(size_t)r] = r; tm[(size_t)r] = r / 60.0; for (int c = 0; c < 7; ++c) dat[(size_t)r * 7 + c] = (r % 9 == 0) ? 0.0 / 0.0 : r * 1e-3 * (c - 3); }
            if (p2s_trc_append_rows(trc, 100, 7, fr.data(), tm.data(), dat.data(), threads) != P2S_OK) return 9;
        }
    }
    if (argc > 4) {                                    // OpenPose files: 2 cameras x 70 frames x 3 markers
        const std::string dirs = std::string(argv[3]) + argv[4];
        const int64_t doff[3] = {0, (int64_t)strlen(argv[3]), (int64_t)dirs.size()};
        const int32_t order[3] = {2, 0, 1};
        std::vector<double> uv(2 * 70 * 3 * 2);
        for (size_t i = 0; i < uv.size(); ++i) uv[i] = i % 13 == 0 ? 0.0 / 0.0 : (double)(i % 97) * 7.5;
        int64_t n_written = 0;
        if (p2s_write_openpose_files(dirs.data(), doff, "trial", 2, 70, 3, 3, order, uv.data(), threads, &n_written) != P2S_OK) return 15;
        if (n_written != 140) return 16;
    }
    {                                                  // proposals: 600 frames of 3 cameras, at most 8 detections a frame
        const int64_t F = 600;
        const int32_t C = 3, M = 8;
        std::vector<int32_t> np_((size_t)F * C), rows_((size_t)F * M * C), n_rows((size_t)F), uniq((size_t)F * M * C), n_uniq((size_t)F),
            rank((size_t)F * M), props((size_t)F * M * C), n_props((size_t)F);
        std::vector<int64_t> cnt((size_t)F * M);
        std::vector<double> aff((size_t)F * M * M);
        for (int64_t f = 0; f < F; ++f) {
            np_[(size_t)f * C + 0] = (int32_t)(f % 3);
            np_[(size_t)f * C + 1] = (int32_t)(f / 3 % 4);
            np_[(size_t)f * C + 2] = 2;
            n_rows[(size_t)f] = np_[(size_t)f * C] + np_[(size_t)f * C + 1] + 2;
            for (int i = 0; i < M; ++i) rank[(size_t)f * M + i] = i;
            for (int i = 0; i < M * M; ++i) aff[(size_t)f * M * M + i] = (f + i) % 29 == 0 ? 0.0 / 0.0 : (double)((f * 7 + i * 5) % 11) / 10.0 - 0.2;
        }
        if (p2s_assoc_argmax_rows(F, C, M, aff.data(), np_.data(), threads, rows_.data()) != P2S_OK) return 17;
        if (p2s_assoc_unique_rows(F, C, M, rows_.data(), n_rows.data(), threads, uniq.data(), cnt.data(), n_uniq.data()) != P2S_OK) return 18;
        if (p2s_assoc_filter_rows(F, C, M, uniq.data(), n_uniq.data(), rank.data(), 2, threads, props.data(), n_props.data()) != P2S_OK) return 19;
    }
    long ok = 0;
    for (int64_t i = 0; i < n; ++i) ok += counts[(size_t)i] >= 0;
    printf("files %lld readable %ld people %lld\n", (long long)n, ok, (long long)base[(size_t)n]);
    p2s_json_free(b);
    return 0;
}
