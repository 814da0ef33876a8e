// .trc data rows (host side of the C-ABI, include/p2s.h): the text DataFrame.to_csv(sep='\t', header=None,
// lineterminator='\n') writes in the reference's make_trc (triangulation.py:214) -- one line per frame,
// `frame \t time \t v1 \t v2 ...`, floats as Python's repr() prints them (shortest digits that round-trip, fixed
// notation for 1e-4 <= |v| < 1e16, otherwise d.ddde+XX), NaN as an empty field.  pandas formats every value
// through a Python object; at 100 k frames x 78 columns that is ~20 s, this writer takes a fraction of a second.
// Also the rows of Utilities/confidence_timeline.py's CSV (p2s_timeline_write_csv): csv.writer's text, NaN as 'nan'.
#include <algorithm>
#include <cerrno>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <atomic>

#include "p2s.h"
#include "p2s_error.h"
#include "p2s_host.h"

namespace {

// repr(float): CPython's float_repr_style 'short' (format_float_short with 'r'): shortest round-trip digits,
// decimal point position decpt; exponent form when decpt <= -4 or decpt > 16, else fixed with at least '.0'.
inline char *py_repr(char *out, double v) {
    if (v != v) return out;                                   // NaN: na_rep = ''
    if (std::isinf(v)) {
        if (v < 0) *out++ = '-';
        memcpy(out, "inf", 3);
        return out + 3;
    }
    if (std::signbit(v)) { *out++ = '-'; v = -v; }
    if (v == 0.0) { memcpy(out, "0.0", 3); return out + 3; }
    char buf[40];
    const auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::scientific);   // d[.ddd]e[+-]XX, shortest
    char *e = buf;
    while (*e != 'e') ++e;
    // digits without the point
    char digits[24];
    int nd = 0;
    for (char *p = buf; p < e; ++p)
        if (*p != '.') digits[nd++] = *p;
    int exp10 = 0;
    {
        const char *p = e + 1;
        const bool neg = *p == '-';
        if (*p == '+' || *p == '-') ++p;
        for (; p < r.ptr; ++p) exp10 = exp10 * 10 + (*p - '0');
        if (neg) exp10 = -exp10;
    }
    const int decpt = exp10 + 1;                              // value = 0.d1d2... x 10^decpt
    if (decpt <= -4 || decpt > 16) {                          // exponent form: d[.ddd]e+XX (at least two exponent digits)
        *out++ = digits[0];
        if (nd > 1) {
            *out++ = '.';
            memcpy(out, digits + 1, (size_t)nd - 1);
            out += nd - 1;
        }
        *out++ = 'e';
        int x = decpt - 1;
        *out++ = x < 0 ? '-' : '+';
        if (x < 0) x = -x;
        char t[8];
        int n = 0;
        while (x) { t[n++] = (char)('0' + x % 10); x /= 10; }
        while (n < 2) t[n++] = '0';
        while (n) *out++ = t[--n];
        return out;
    }
    if (decpt <= 0) {                                         // 0.000ddd
        *out++ = '0';
        *out++ = '.';
        for (int i = 0; i < -decpt; ++i) *out++ = '0';
        memcpy(out, digits, (size_t)nd);
        return out + nd;
    }
    if (decpt >= nd) {                                        // ddd000.0
        memcpy(out, digits, (size_t)nd);
        out += nd;
        for (int i = nd; i < decpt; ++i) *out++ = '0';
        *out++ = '.';
        *out++ = '0';
        return out;
    }
    memcpy(out, digits, (size_t)decpt);                       // dd.ddd
    out += decpt;
    *out++ = '.';
    memcpy(out, digits + decpt, (size_t)(nd - decpt));
    return out + (nd - decpt);
}

inline char *put_int(char *out, int64_t v) {
    const auto r = std::to_chars(out, out + 24, v);
    return r.ptr;
}

}  // namespace

extern "C" {

int p2s_format_float_repr(double value, char *out, int32_t capacity) {
    if (!out || capacity < 32) return p2s_set_error(P2S_ERR_INVALID_ARG, "buffer of at least 32 bytes required");
    char *e = py_repr(out, value);
    *e = 0;
    return (int)(e - out);
}

int p2s_trc_append_rows(const char *path, int64_t n_rows, int32_t n_cols, const int64_t *frames, const double *time,
                        const double *data, int32_t n_threads) {
    if (!path || n_rows < 0 || n_cols < 0 || (n_rows > 0 && (!frames || !time || (n_cols > 0 && !data))))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "bad arguments");
    FILE *fh = fopen(path, "ab");
    if (!fh) return p2s_set_error(P2S_ERR_INVALID_ARG, "cannot open %s for appending", path);
    const int nt = host_threads(n_threads, 32, 32);           // not clamped to the rows: a group is nt blocks
    const int64_t block = 4096;                               // rows formatted per task
    const size_t row_cap = 48 + (size_t)n_cols * 26;
    int rc = P2S_OK;
    try {
        // blocks are formatted in parallel, a group of nt blocks at a time, and written in order
        std::vector<std::vector<char>> bufs((size_t)nt);
        std::vector<size_t> used((size_t)nt);
        for (int64_t g0 = 0; g0 < n_rows && rc == P2S_OK; g0 += block * nt) {
            const int64_t left = (n_rows - g0 + block - 1) / block;
            const int n_blocks = (int)(left < nt ? left : nt);
            const bool done = parallel_for(n_blocks, n_blocks, 1, [&](int, int64_t slot, int64_t) {
                const int64_t lo = g0 + slot * block;
                const int64_t hi = lo + block < n_rows ? lo + block : n_rows;
                std::vector<char> &b = bufs[(size_t)slot];
                b.resize((size_t)(hi - lo) * row_cap);
                char *o = b.data();
                for (int64_t r = lo; r < hi; ++r) {
                    o = put_int(o, frames[r]);
                    *o++ = '\t';
                    o = py_repr(o, time[r]);
                    const double *row = data + r * (int64_t)n_cols;
                    for (int32_t c = 0; c < n_cols; ++c) {
                        *o++ = '\t';
                        o = py_repr(o, row[c]);
                    }
                    *o++ = '\n';
                }
                used[(size_t)slot] = (size_t)(o - b.data());
            });
            if (!done) throw std::bad_alloc();
            for (int t = 0; t < n_blocks; ++t)
                if (fwrite(bufs[(size_t)t].data(), 1, used[(size_t)t], fh) != used[(size_t)t])
                    rc = p2s_set_error(P2S_ERR_INVALID_ARG, "short write to %s", path);
        }
    } catch (const std::bad_alloc &) {
        rc = p2s_set_error(P2S_ERR_OOM, "out of host memory while formatting");
    }
    if (fclose(fh) != 0 && rc == P2S_OK) rc = p2s_set_error(P2S_ERR_INVALID_ARG, "error closing %s", path);
    return rc;
}

int p2s_timeline_write_csv(const char *path, int64_t n_rows, const int32_t *frame, const int32_t *person, const int32_t *slot,
                           const double *confidence, int32_t n_names, const char *names, const int64_t *name_off, int32_t n_threads) {
    if (!path || n_rows < 0 || n_names < 0 || (n_names > 0 && (!names || !name_off)) || (n_rows > 0 && (!frame || !person || !slot || !confidence)))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "bad arguments");
    size_t longest = 0;
    for (int32_t k = 0; k < n_names; ++k) {
        if (name_off[k + 1] < name_off[k]) return p2s_set_error(P2S_ERR_INVALID_ARG, "name_off must not decrease");
        longest = std::max(longest, (size_t)(name_off[k + 1] - name_off[k]));
        for (int64_t i = name_off[k]; i < name_off[k + 1]; ++i)
            if (names[i] == ',' || names[i] == '"' || names[i] == '\r' || names[i] == '\n')
                return p2s_set_error(P2S_ERR_INVALID_ARG, "name %d holds a character csv.writer would quote", k);
    }
    for (int64_t r = 0; r < n_rows; ++r)
        if (slot[r] < 0 || slot[r] >= n_names) return p2s_set_error(P2S_ERR_INVALID_ARG, "row %lld names slot %d of %d", (long long)r, slot[r], n_names);
    FILE *fh = fopen(path, "wb");
    if (!fh) return p2s_set_error(P2S_ERR_INVALID_ARG, "cannot open %s for writing", path);
    static const char head[] = "frame,person,keypoint,confidence\r\n";
    int rc = fwrite(head, 1, sizeof head - 1, fh) == sizeof head - 1 ? P2S_OK : p2s_set_error(P2S_ERR_INVALID_ARG, "short write to %s", path);
    const int nt = host_threads(n_threads, 32, 32);
    const int64_t block = 16384;                              // rows formatted per task
    const size_t row_cap = 11 + 1 + 11 + 1 + longest + 1 + 25 + 2;
    try {
        // as p2s_trc_append_rows: a group of nt blocks is formatted in parallel and written in order
        std::vector<std::vector<char>> bufs((size_t)nt);
        std::vector<size_t> used((size_t)nt);
        for (int64_t g0 = 0; g0 < n_rows && rc == P2S_OK; g0 += block * nt) {
            const int64_t left = (n_rows - g0 + block - 1) / block;
            const int n_blocks = (int)(left < nt ? left : nt);
            const bool done = parallel_for(n_blocks, n_blocks, 1, [&](int, int64_t b, int64_t) {
                const int64_t lo = g0 + b * block;
                const int64_t hi = lo + block < n_rows ? lo + block : n_rows;
                std::vector<char> &buf = bufs[(size_t)b];
                buf.resize((size_t)(hi - lo) * row_cap);
                char *o = buf.data();
                for (int64_t r = lo; r < hi; ++r) {
                    o = put_int(o, frame[r]);
                    *o++ = ',';
                    o = put_int(o, person[r]);
                    *o++ = ',';
                    const size_t len = (size_t)(name_off[slot[r] + 1] - name_off[slot[r]]);
                    memcpy(o, names + name_off[slot[r]], len);
                    o += len;
                    *o++ = ',';
                    if (confidence[r] != confidence[r]) { memcpy(o, "nan", 3); o += 3; }      // repr(float('nan')), whatever its sign
                    else o = py_repr(o, confidence[r]);
                    *o++ = '\r';
                    *o++ = '\n';
                }
                used[(size_t)b] = (size_t)(o - buf.data());
            });
            if (!done) throw std::bad_alloc();
            for (int t = 0; t < n_blocks; ++t)
                if (fwrite(bufs[(size_t)t].data(), 1, used[(size_t)t], fh) != used[(size_t)t])
                    rc = p2s_set_error(P2S_ERR_INVALID_ARG, "short write to %s", path);
        }
    } catch (const std::bad_alloc &) {
        rc = p2s_set_error(P2S_ERR_OOM, "out of host memory while formatting");
    }
    if (fclose(fh) != 0 && rc == P2S_OK) rc = p2s_set_error(P2S_ERR_INVALID_ARG, "error closing %s", path);
    return rc;
}

int p2s_write_openpose_files(const char *dir_paths, const int64_t *dir_offsets, const char *name_root, int32_t n_cams,
                             int64_t n_frames, int32_t n_markers, int32_t n_out, const int32_t *marker_index,
                             const double *uv, int32_t n_threads, int64_t *n_written) {
    if (n_written) *n_written = 0;
    if (n_cams < 0 || n_frames < 0 || n_markers < 0 || n_out < 0 || !name_root || (n_cams > 0 && (!dir_paths || !dir_offsets)) ||
        (n_out > 0 && !marker_index) || (n_cams > 0 && n_frames > 0 && n_out > 0 && !uv))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "bad arguments");
    for (int32_t i = 0; i < n_out; ++i)
        if (marker_index[i] < 0 || marker_index[i] >= n_markers)
            return p2s_set_error(P2S_ERR_INVALID_ARG, "output position %d names marker %d of %d", i, marker_index[i], n_markers);
    const int64_t n_files = (int64_t)n_cams * n_frames;
    if (n_files == 0) return P2S_OK;
    const int64_t grain = 64;
    const int nt = host_threads(n_threads, 16, (n_files + grain - 1) / grain);   // file writing: never more than 16 host threads
    static const char head[] = "{\"version\": 1.3, \"people\": [{\"person_id\": [-1], \"pose_keypoints_2d\": [";
    static const char tail[] = "], \"face_keypoints_2d\": [], \"hand_left_keypoints_2d\": [], \"hand_right_keypoints_2d\": [], "
                               "\"pose_keypoints_3d\": [], \"face_keypoints_3d\": [], \"hand_left_keypoints_3d\": [], "
                               "\"hand_right_keypoints_3d\": []}]}";
    std::atomic<int64_t> done{0}, first_bad{n_files};
    std::vector<int> errs((size_t)nt, 0);
    std::vector<std::string> bad_path((size_t)nt);
    std::vector<int64_t> bad_file((size_t)nt, n_files);
    const bool all_run = parallel_for(n_files, nt, grain, [&](int t, int64_t lo, int64_t hi) {
        std::vector<char> buf(sizeof head + sizeof tail + (size_t)n_out * 64);
        std::string path;
        char num[32];
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t c = i / n_frames, f = i % n_frames;
            char *o = buf.data();
            memcpy(o, head, sizeof head - 1);
            o += sizeof head - 1;
            const double *row = uv + (c * n_frames + f) * (int64_t)n_markers * 2;
            for (int32_t k = 0; k < n_out; ++k) {
                const double x = row[2 * marker_index[k]], y = row[2 * marker_index[k] + 1];
                if (k) { *o++ = ','; *o++ = ' '; }
                if (x != x || y != y) {
                    memcpy(o, "0.0, 0.0, 0", 11);
                    o += 11;
                } else {
                    o = py_repr(o, x);
                    *o++ = ','; *o++ = ' ';
                    o = py_repr(o, y);
                    memcpy(o, ", 1", 3);
                    o += 3;
                }
            }
            memcpy(o, tail, sizeof tail - 1);
            o += sizeof tail - 1;
            path.assign(dir_paths + dir_offsets[c], (size_t)(dir_offsets[c + 1] - dir_offsets[c]));
            path += '/';
            path += name_root;
            snprintf(num, sizeof num, "_cam%02d_openpose_%04lld.json", (int)(c + 1), (long long)f);
            path += num;
            FILE *fh = fopen(path.c_str(), "wb");
            const size_t n = (size_t)(o - buf.data());
            bool ok = fh != nullptr;
            int err = ok ? 0 : errno;
            if (ok && fwrite(buf.data(), 1, n, fh) != n) { ok = false; err = errno; }
            if (fh && fclose(fh) != 0 && ok) { ok = false; err = errno; }
            if (ok) {
                done.fetch_add(1);
            } else if (i < bad_file[(size_t)t]) {
                bad_file[(size_t)t] = i; errs[(size_t)t] = err; bad_path[(size_t)t] = path;
                int64_t cur = first_bad.load();
                while (i < cur && !first_bad.compare_exchange_weak(cur, i)) {}
            }
        }
    });
    if (n_written) *n_written = done.load();
    if (!all_run) return p2s_set_error(P2S_ERR_OOM, "out of host memory while formatting");
    const int64_t bad = first_bad.load();
    if (bad < n_files)
        for (int t = 0; t < nt; ++t)
            if (bad_file[(size_t)t] == bad)
                return p2s_set_error(P2S_ERR_INVALID_ARG, "cannot write %s: %s", bad_path[(size_t)t].c_str(), strerror(errs[(size_t)t]));
    return P2S_OK;
}

}  // extern "C"
