// OpenPose-JSON ingest for the triangulation / association path (host side of the C-ABI, include/p2s.h).
//
// Replaces the per-frame, per-person json.load calls of the reference -- extract_files_frame_f
// (triangulation.py:607-653), count_persons_in_json (:77-90), read_json (personAssociation.py:260-274) --
// by one pass over all files on host threads: every file is read and parsed ONCE into a per-thread
// arena, and the gather calls then lay the numbers out the way the kernels consume them.
//
// The parser accepts exactly the documents Python's json.load accepts (RFC 8259 plus the NaN / Infinity /
// -Infinity literals, strict control-character and UTF-8 checks, duplicate keys -> last one wins) so that a
// file the reference would treat as unreadable is unreadable here too, and converts numbers with
// std::from_chars, which is correctly rounded like Python's float().
#include <atomic>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include <errno.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "p2s.h"
#include "p2s_error.h"
#include "p2s_host.h"
#include "p2s_npsum_small.h"

namespace {

constexpr int kMaxDepth = 256;

enum PersonStatus : int8_t {
    kPersonOk = 0,        // object with a "pose_keypoints_2d" array of numbers
    kPersonNoList = 1,    // not an object, key missing, or the value is not an array
    kPersonNonNumeric = 2, // array holding something that is not a number / null / bool
    kPersonBadList = 3    // object whose "pose_keypoints_2d" is not an array (read as kPersonNoList except by the
                          // synchronization gather: indexing that value raises in the reference)
};

enum : int8_t { kPersonNotObject = 1, kPersonHasNull = 2, kPersonAllInts = 4, kPersonHasBool = 8, kPersonBigInt = 16 };   // Person::flags
enum : int8_t { kFileTopObject = 1, kFilePeopleNull = 2, kFilePeopleOther = 4 };  // FileRec::flags; bits 3..5: kFileTopShift
constexpr int kFileTopShift = 3;      // (P2S_JSON_DOC_LIST .. P2S_JSON_DOC_NULL) - P2S_JSON_DOC_LIST + 1 of a document that is no object

struct Person {
    int64_t off;
    int32_t len;
    int8_t status;
    int8_t flags;         // what the status does not tell apart (p2s_json_select_tracked_person)
    int32_t id_len = 0;   // the raw text of the "person_id" value in Arena::texts, 0 bytes = no such key
    int64_t id_off = 0;
};

struct FileRec {
    int32_t count;        // >= 0: len(people); P2S_JSON_UNREADABLE; P2S_JSON_NO_PEOPLE_LIST
    int32_t thread;
    int64_t first_person; // index into the thread's person vector
    int8_t flags;         // kFile*: why a valid document has no "people" list
};

struct Arena {
    std::vector<double> values;
    std::vector<Person> persons;
    std::vector<char> texts;
    std::vector<char> buf;
};

struct Parser {
    const char *p, *end;
    Arena *arena;
    bool ok = true;
    bool number_is_int = false;   // the last number() had neither fraction nor exponent: Python reads an int
    // result for the current file
    bool have_people = false;
    size_t people_first = 0;
    int32_t people_count = 0;
    int8_t file_flags = 0;

    inline void ws() {
        while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) ++p;
    }
    bool fail() {
        ok = false;
        return false;
    }
    static int hexval(char c) {
        if (c >= '0' && c <= '9') return c - '0';
        if (c >= 'a' && c <= 'f') return c - 'a' + 10;
        if (c >= 'A' && c <= 'F') return c - 'A' + 10;
        return -1;
    }
    // p at the opening quote.  key != nullptr: the unescaped bytes (only needed to compare object keys;
    // \u escapes beyond ASCII are stored as '?', none of the wanted keys has them).
    bool string(std::string *key) {
        ++p;
        if (key) key->clear();
        while (true) {
            if (p >= end) return fail();
            const unsigned char c = (unsigned char)*p;
            if (c == '"') {
                ++p;
                return true;
            }
            if (c < 0x20) return fail();             // json.loads(strict=True)
            if (c == '\\') {
                if (p + 1 >= end) return fail();
                const char e = p[1];
                char out;
                switch (e) {
                    case '"': out = '"'; break;
                    case '\\': out = '\\'; break;
                    case '/': out = '/'; break;
                    case 'b': out = '\b'; break;
                    case 'f': out = '\f'; break;
                    case 'n': out = '\n'; break;
                    case 'r': out = '\r'; break;
                    case 't': out = '\t'; break;
                    case 'u': {
                        if (p + 6 > end) return fail();
                        int v = 0;
                        for (int i = 2; i < 6; ++i) {
                            const int h = hexval(p[i]);
                            if (h < 0) return fail();
                            v = v * 16 + h;
                        }
                        out = v < 0x80 ? (char)v : '?';
                        p += 4;
                        break;
                    }
                    default: return fail();
                }
                if (key) key->push_back(out);
                p += 2;
                continue;
            }
            if (key) key->push_back((char)c);
            ++p;
        }
    }
    // JSON number at p (first char is '-' or a digit).  value == nullptr: validate only.
    bool number(double *value) {
        const char *s = p;
        if (p < end && *p == '-') ++p;
        if (p >= end) return fail();
        if (*p == '0') {
            ++p;
        } else if (*p >= '1' && *p <= '9') {
            while (p < end && *p >= '0' && *p <= '9') ++p;
        } else {
            return fail();
        }
        const char *int_end = p;
        if (p + 1 < end && *p == '.' && p[1] >= '0' && p[1] <= '9') {     // a lone '.' ends the number (-> error later)
            ++p;
            while (p < end && *p >= '0' && *p <= '9') ++p;
        }
        if (p < end && (*p == 'e' || *p == 'E')) {
            const char *q = p + 1;
            if (q < end && (*q == '+' || *q == '-')) ++q;
            if (q < end && *q >= '0' && *q <= '9') {
                while (q < end && *q >= '0' && *q <= '9') ++q;
                p = q;
            }                                                               // else: "1e" -> number ends before 'e'
        }
        number_is_int = p == int_end;
        if (!value) return true;
        double d = 0.0;
        const auto r = std::from_chars(s, p, d);
        if (r.ec == std::errc::result_out_of_range) {
            // float('1e999') = inf, float('1e-999') = 0.0; an integer literal that large cannot be an array
            // element NumPy converts, but inf keeps the slot numeric.
            bool neg_exp = false;
            for (const char *q = int_end; q < p; ++q)
                if ((*q == 'e' || *q == 'E') && q + 1 < p && q[1] == '-') neg_exp = true;
            d = neg_exp ? 0.0 : std::numeric_limits<double>::infinity();
            if (*s == '-') d = -d;
        } else if (r.ec != std::errc()) {
            return fail();
        }
        *value = d;
        return true;
    }
    bool literal(const char *word) {
        const size_t n = strlen(word);
        if ((size_t)(end - p) < n || memcmp(p, word, n) != 0) return fail();
        p += n;
        return true;
    }
    // Any JSON value, validated and skipped.
    bool skip(int depth) {
        if (depth > kMaxDepth) return fail();
        ws();
        if (p >= end) return fail();
        switch (*p) {
            case '{': {
                ++p;
                ws();
                if (p < end && *p == '}') {
                    ++p;
                    return true;
                }
                while (true) {
                    ws();
                    if (p >= end || *p != '"') return fail();
                    if (!string(nullptr)) return false;
                    ws();
                    if (p >= end || *p != ':') return fail();
                    ++p;
                    if (!skip(depth + 1)) return false;
                    ws();
                    if (p < end && *p == ',') {
                        ++p;
                        continue;
                    }
                    if (p < end && *p == '}') {
                        ++p;
                        return true;
                    }
                    return fail();
                }
            }
            case '[': {
                ++p;
                ws();
                if (p < end && *p == ']') {
                    ++p;
                    return true;
                }
                while (true) {
                    if (!skip(depth + 1)) return false;
                    ws();
                    if (p < end && *p == ',') {
                        ++p;
                        continue;
                    }
                    if (p < end && *p == ']') {
                        ++p;
                        return true;
                    }
                    return fail();
                }
            }
            case '"': return string(nullptr);
            case 't': return literal("true");
            case 'f': return literal("false");
            case 'n': return literal("null");
            case 'N': return literal("NaN");
            case 'I': return literal("Infinity");
            case '-':
                if (p + 1 < end && p[1] == 'I') {
                    ++p;
                    return literal("Infinity");
                }
                return number(nullptr);
            default:
                if (*p >= '0' && *p <= '9') return number(nullptr);
                return fail();
        }
    }
    // The value of a "pose_keypoints_2d" key.
    bool keypoint_list(Person &person) {
        ws();
        if (p >= end) return fail();
        if (*p != '[') {
            person.status = kPersonBadList;
            person.len = 0;
            return skip(3);
        }
        ++p;
        std::vector<double> &v = arena->values;
        person.off = (int64_t)v.size();
        person.status = kPersonOk;
        person.flags &= (int8_t)~(kPersonHasNull | kPersonAllInts | kPersonHasBool | kPersonBigInt);
        bool all_ints = true;
        ws();
        if (p < end && *p == ']') {
            ++p;
            person.len = 0;
            return true;
        }
        const double nan = std::numeric_limits<double>::quiet_NaN();
        while (true) {
            ws();
            if (p >= end) return fail();
            const char c = *p;
            double d;
            number_is_int = false;                         // stays so for every literal
            if ((c >= '0' && c <= '9') || (c == '-' && !(p + 1 < end && p[1] == 'I'))) {
                const char *token = p;
                if (!number(&d)) return false;
                if (number_is_int) {                       // an integer float64 does not hold exactly: beyond +-2^53
                    long long exact = 0;
                    const auto r = std::from_chars(token, p, exact);
                    if (r.ec != std::errc() || exact > (1LL << 53) || exact < -(1LL << 53)) person.flags |= kPersonBigInt;
                }
            } else if (c == 'N') {
                if (!literal("NaN")) return false;
                d = nan;
            } else if (c == 'I') {
                if (!literal("Infinity")) return false;
                d = std::numeric_limits<double>::infinity();
            } else if (c == '-') {
                ++p;
                if (!literal("Infinity")) return false;
                d = -std::numeric_limits<double>::infinity();
            } else if (c == 'n') {
                if (!literal("null")) return false;
                d = nan;                                   // numpy: float(None) -> nan
                person.flags |= kPersonHasNull;
            } else if (c == 't') {
                if (!literal("true")) return false;
                d = 1.0;
                person.flags |= kPersonHasBool;
            } else if (c == 'f') {
                if (!literal("false")) return false;
                d = 0.0;
                person.flags |= kPersonHasBool;
            } else {
                if (!skip(4)) return false;                // string / array / object: not a number list
                person.status = kPersonNonNumeric;
                number_is_int = false;                     // whatever the skipped value held
                d = nan;
            }
            all_ints &= number_is_int;
            v.push_back(d);
            ws();
            if (p < end && *p == ',') {
                ++p;
                continue;
            }
            if (p < end && *p == ']') {
                ++p;
                break;
            }
            return fail();
        }
        person.len = (int32_t)((int64_t)v.size() - person.off);
        if (all_ints) person.flags |= kPersonAllInts;
        return true;
    }
    // One element of the "people" array.
    bool person(std::string &key) {
        Person rec{0, 0, kPersonNoList, 0, 0, 0};
        ws();
        if (p >= end) return fail();
        if (*p != '{') {
            rec.flags = kPersonNotObject;
            if (!skip(2)) return false;
            arena->persons.push_back(rec);
            return true;
        }
        ++p;
        ws();
        if (p < end && *p == '}') {
            ++p;
            arena->persons.push_back(rec);
            return true;
        }
        while (true) {
            ws();
            if (p >= end || *p != '"') return fail();
            if (!string(&key)) return false;
            ws();
            if (p >= end || *p != ':') return fail();
            ++p;
            if (key == "pose_keypoints_2d") {
                if (!keypoint_list(rec)) return false;     // a repeated key overrides (dict semantics)
            } else if (key == "person_id") {
                ws();
                const char *first = p;
                if (!skip(3)) return false;
                rec.id_off = (int64_t)arena->texts.size();
                rec.id_len = (int32_t)(p - first);
                arena->texts.insert(arena->texts.end(), first, p);
            } else if (!skip(3)) {
                return false;
            }
            ws();
            if (p < end && *p == ',') {
                ++p;
                continue;
            }
            if (p < end && *p == '}') {
                ++p;
                break;
            }
            return fail();
        }
        arena->persons.push_back(rec);
        return true;
    }
    // The value of the top-level "people" key.
    bool people(std::string &key) {
        ws();
        if (p >= end) return fail();
        arena->persons.resize(people_first);                // a repeated "people" key overrides
        people_count = 0;
        file_flags &= (int8_t)~(kFilePeopleNull | kFilePeopleOther);
        if (*p != '[') {
            have_people = false;
            file_flags |= *p == 'n' ? kFilePeopleNull : kFilePeopleOther;
            return skip(1);
        }
        have_people = true;
        ++p;
        ws();
        if (p < end && *p == ']') {
            ++p;
            return true;
        }
        while (true) {
            if (!person(key)) return false;
            ++people_count;
            ws();
            if (p < end && *p == ',') {
                ++p;
                continue;
            }
            if (p < end && *p == ']') {
                ++p;
                return true;
            }
            return fail();
        }
    }
    // Whole document.  Returns the FileRec count field.
    int32_t document() {
        std::string key;
        people_first = arena->persons.size();
        const size_t values_first = arena->values.size(), texts_first = arena->texts.size();
        ws();
        bool is_object = false;
        if (p < end && *p == '{') {
            is_object = true;
            file_flags |= kFileTopObject;
            ++p;
            ws();
            if (p < end && *p == '}') {
                ++p;
            } else {
                while (ok) {
                    ws();
                    if (p >= end || *p != '"') {
                        fail();
                        break;
                    }
                    if (!string(&key)) break;
                    ws();
                    if (p >= end || *p != ':') {
                        fail();
                        break;
                    }
                    ++p;
                    if (key == "people") {
                        if (!people(key)) break;
                    } else if (!skip(1)) {
                        break;
                    }
                    ws();
                    if (p < end && *p == ',') {
                        ++p;
                        continue;
                    }
                    if (p < end && *p == '}') {
                        ++p;
                        break;
                    }
                    fail();
                }
            }
        } else {
            int top = P2S_JSON_DOC_FLOAT;                    // what type(json.load(f)) will be
            if (p < end) {
                const char c = *p;
                if (c == '[') top = P2S_JSON_DOC_LIST;
                else if (c == '"') top = P2S_JSON_DOC_STRING;
                else if (c == 't' || c == 'f') top = P2S_JSON_DOC_BOOL;
                else if (c == 'n') top = P2S_JSON_DOC_NULL;
            }
            const char *first = p;
            skip(0);
            if (ok && top == P2S_JSON_DOC_FLOAT && first < p && *first != 'N' && *first != 'I' && !(*first == '-' && first + 1 < p && first[1] == 'I')) {
                top = P2S_JSON_DOC_INT;                      // a number without fraction and exponent
                for (const char *q = first; q < p; ++q)
                    if (*q == '.' || *q == 'e' || *q == 'E') top = P2S_JSON_DOC_FLOAT;
            }
            file_flags |= (int8_t)((top - P2S_JSON_DOC_LIST + 1) << kFileTopShift);
        }
        if (ok) {
            ws();
            if (p != end) ok = false;                       // json: "Extra data"
        }
        if (!ok || !is_object || !have_people) {
            arena->persons.resize(people_first);
            arena->values.resize(values_first);
            arena->texts.resize(texts_first);
            return ok ? P2S_JSON_NO_PEOPLE_LIST : P2S_JSON_UNREADABLE;
        }
        return people_count;
    }
};

}  // namespace

struct p2s_json_batch {
    int64_t n_files = 0;
    int n_threads = 1;
    std::vector<FileRec> files;
    std::vector<Arena> arenas;
    std::vector<int64_t> person_base;   // [n_files + 1]: prefix sums of max(count, 0)
};

extern "C" {

int p2s_json_parse(const char *paths, const int64_t *path_offsets, int64_t n_files, int32_t n_threads,
                   p2s_json_batch **out) {
    if (!out) return p2s_set_error(P2S_ERR_INVALID_ARG, "null output handle");
    *out = nullptr;
    if (n_files < 0 || (n_files > 0 && (!paths || !path_offsets)))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "bad path table");
    for (int64_t i = 0; i < n_files; ++i)
        if (path_offsets[i + 1] < path_offsets[i]) return p2s_set_error(P2S_ERR_INVALID_ARG, "path offsets must not decrease");
    p2s_json_batch *b = new (std::nothrow) p2s_json_batch();
    if (!b) return p2s_set_error(P2S_ERR_OOM, "out of host memory");
    try {
        b->n_files = n_files;
        b->n_threads = host_threads(n_threads, 64, n_files / 64 + 1);
        b->files.resize((size_t)n_files);
        b->arenas.resize((size_t)b->n_threads);
        const bool done = parallel_for(n_files, b->n_threads, 64, [&](int t, int64_t lo, int64_t hi) {
            Arena &arena = b->arenas[(size_t)t];
            std::string path;
            for (int64_t i = lo; i < hi; ++i) {
                FileRec &fr = b->files[(size_t)i];
                fr.thread = t;
                fr.first_person = (int64_t)arena.persons.size();
                fr.count = P2S_JSON_UNREADABLE;
                fr.flags = 0;
                const int64_t len = path_offsets[i + 1] - path_offsets[i];
                if (len <= 0) continue;                                     // no file for this slot
                path.assign(paths + path_offsets[i], (size_t)len);
                size_t n = 0;
                if (!read_file(path.c_str(), arena.buf, n)) continue;
                if (!valid_utf8((const unsigned char *)arena.buf.data(), n)) continue;
                Parser ps;
                ps.p = arena.buf.data();
                ps.end = ps.p + n;
                ps.arena = &arena;
                fr.count = ps.document();
                fr.flags = ps.file_flags;
            }
        });
        if (!done) throw std::bad_alloc();
        b->person_base.resize((size_t)n_files + 1);
        b->person_base[0] = 0;
        for (int64_t i = 0; i < n_files; ++i)
            b->person_base[(size_t)i + 1] = b->person_base[(size_t)i] + (b->files[(size_t)i].count > 0 ? b->files[(size_t)i].count : 0);
    } catch (const std::bad_alloc &) {
        delete b;
        return p2s_set_error(P2S_ERR_OOM, "out of host memory while parsing");
    }
    *out = b;
    return P2S_OK;
}

int p2s_json_free(p2s_json_batch *b) {
    delete b;
    return P2S_OK;
}

int p2s_json_people_counts(const p2s_json_batch *b, int32_t *counts, int64_t *person_base) {
    if (!b) return p2s_set_error(P2S_ERR_INVALID_ARG, "null batch");
    for (int64_t i = 0; i < b->n_files; ++i) {
        if (counts) counts[i] = b->files[(size_t)i].count;
        if (person_base) person_base[i] = b->person_base[(size_t)i];
    }
    if (person_base) person_base[b->n_files] = b->person_base[(size_t)b->n_files];
    return P2S_OK;
}

int p2s_json_person_lengths(const p2s_json_batch *b, int32_t *lengths) {
    if (!b || !lengths) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    for (int64_t i = 0; i < b->n_files; ++i) {
        const FileRec &fr = b->files[(size_t)i];
        const Arena &arena = b->arenas[(size_t)fr.thread];
        for (int32_t n = 0; n < fr.count; ++n) {
            const Person &ps = arena.persons[(size_t)(fr.first_person + n)];
            lengths[b->person_base[(size_t)i] + n] =
                ps.status == kPersonOk ? ps.len : (ps.status == kPersonNoList || ps.status == kPersonBadList ? P2S_JSON_PERSON_NO_LIST : P2S_JSON_PERSON_NOT_NUMERIC);
        }
    }
    return P2S_OK;
}

int p2s_json_person_flags(const p2s_json_batch *b, int32_t *flags) {
    if (!b || !flags) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    for (int64_t i = 0; i < b->n_files; ++i) {
        const FileRec &fr = b->files[(size_t)i];
        const Arena &arena = b->arenas[(size_t)fr.thread];
        for (int32_t n = 0; n < fr.count; ++n) {
            const Person &ps = arena.persons[(size_t)(fr.first_person + n)];
            const bool list = ps.status == kPersonOk || ps.status == kPersonNonNumeric;
            flags[b->person_base[(size_t)i] + n] =
                (list && ps.len > 0 && (ps.flags & kPersonAllInts) ? P2S_JSON_PERSON_ALL_INTS : 0) |
                (list && (ps.flags & kPersonHasNull) ? P2S_JSON_PERSON_HAS_NULL : 0) |
                (list && (ps.flags & kPersonHasBool) ? P2S_JSON_PERSON_HAS_BOOL : 0) |
                (list && (ps.flags & kPersonBigInt) ? P2S_JSON_PERSON_BIG_INT : 0) |
                ((ps.flags & kPersonNotObject) ? P2S_JSON_PERSON_NOT_OBJECT : 0) |
                (ps.status == kPersonBadList ? P2S_JSON_PERSON_BAD_LIST : 0);
        }
    }
    return P2S_OK;
}

}  // extern "C"

namespace {

template <typename T>
inline void store_value(T *dst, double v, int64_t &inexact) {
    const T t = (T)v;
    if (sizeof(T) == 4 && (double)t != v && v == v) ++inexact;
    *dst = t;
}

// The gathers return how many values float32 cannot hold exactly, -1 when a worker ran out of memory.
template <typename T>
int64_t gather_keypoints(const p2s_json_batch *b, const int32_t *ids, int32_t n_ids, int32_t max_persons,
                         const int64_t *file_offsets, int64_t person_stride, T *out) {
    std::atomic<int64_t> inexact_total{0};
    const T nan = std::numeric_limits<T>::quiet_NaN();
    const bool done = parallel_for(b->n_files, host_threads(b->n_threads, 64, b->n_files / 256 + 1), 256, [&](int, int64_t lo, int64_t hi) {
        int64_t inexact = 0;
        for (int64_t i = lo; i < hi; ++i) {
            const FileRec &fr = b->files[(size_t)i];
            const Arena &arena = b->arenas[(size_t)fr.thread];
            if (file_offsets[i] < 0) continue;
            for (int32_t n = 0; n < max_persons; ++n) {
                T *dst = out + file_offsets[i] + (int64_t)n * person_stride;
                const Person *ps = n < fr.count ? &arena.persons[(size_t)(fr.first_person + n)] : nullptr;
                const bool usable = ps && ps->status == kPersonOk;
                const double *src = usable ? arena.values.data() + ps->off : nullptr;
                for (int32_t k = 0; k < n_ids; ++k) {
                    const int64_t j = (int64_t)ids[k] * 3;
                    if (usable && ids[k] >= 0 && j + 2 < ps->len) {        // the whole triplet exists (:631-639)
                        store_value(dst + 3 * k + 0, src[j + 0], inexact);
                        store_value(dst + 3 * k + 1, src[j + 1], inexact);
                        store_value(dst + 3 * k + 2, src[j + 2], inexact);
                    } else {
                        dst[3 * k + 0] = nan;
                        dst[3 * k + 1] = nan;
                        dst[3 * k + 2] = nan;
                    }
                }
            }
        }
        inexact_total.fetch_add(inexact);
    });
    return done ? inexact_total.load() : -1;
}

template <typename T>
int64_t gather_people(const p2s_json_batch *b, const int64_t *file_of, const int32_t *person_of, int64_t n_rows,
                      int32_t n_values, T *out) {
    std::atomic<int64_t> inexact_total{0};
    const T nan = std::numeric_limits<T>::quiet_NaN();
    const bool done = parallel_for(n_rows, host_threads(b->n_threads, 64, n_rows / 1024 + 1), 1024, [&](int, int64_t lo, int64_t hi) {
        int64_t inexact = 0;
        for (int64_t r = lo; r < hi; ++r) {
            T *dst = out + r * (int64_t)n_values;
            const FileRec &fr = b->files[(size_t)file_of[r]];
            const Arena &arena = b->arenas[(size_t)fr.thread];
            const Person &ps = arena.persons[(size_t)(fr.first_person + person_of[r])];
            const double *src = arena.values.data() + ps.off;
            const int32_t n = ps.status == kPersonOk ? (ps.len < n_values ? ps.len : n_values) : 0;
            for (int32_t k = 0; k < n; ++k) store_value(dst + k, src[k], inexact);
            for (int32_t k = n; k < n_values; ++k) dst[k] = nan;
        }
        inexact_total.fetch_add(inexact);
    });
    return done ? inexact_total.load() : -1;
}


// convert_json2pandas (synchronization.py:1185-1250) on one parsed file; false where the reference's try block raises.
bool largest_person(const p2s_json_batch *b, int64_t i, const int32_t *ids, int32_t n_ids, double thr, double *dst) {
    const FileRec &fr = b->files[(size_t)i];
    if (fr.count <= 0) return false;                                  // no "people" list / np.argmax of an empty list
    const Arena &arena = b->arenas[(size_t)fr.thread];
    int32_t best = -1;
    double best_area = 0.0;
    for (int32_t n = 0; n < fr.count; ++n) {
        // the comprehension of :1219-1224 indexes p['pose_keypoints_2d'] before its `in p` test: a person without a
        // list of numbers (or not an object) raises, whatever its place
        const Person &ps = arena.persons[(size_t)(fr.first_person + n)];
        if (ps.status != kPersonOk || n_ids == 0) return false;      // (no keypoint: max() of an empty array)
        const double *v = arena.values.data() + ps.off;
        double x_lo = 0, x_hi = 0, y_lo = 0, y_hi = 0;
        bool nan = false;
        for (int32_t k = 0; k < n_ids; ++k) {
            const int64_t j = (int64_t)ids[k] * 3;
            if (ids[k] < 0 || j + 2 >= ps.len) return false;          // a short slice: ragged array / IndexError
            const double x = v[j], y = v[j + 1];
            if (x != x || y != y) nan = true;
            if (k == 0) { x_lo = x_hi = x; y_lo = y_hi = y; }
            x_lo = std::fmin(x_lo, x); x_hi = std::fmax(x_hi, x); y_lo = std::fmin(y_lo, y); y_hi = std::fmax(y_hi, y);
        }
        const double area = nan ? std::numeric_limits<double>::quiet_NaN() : (x_hi - x_lo) * (y_hi - y_lo);
        if (best < 0) { best = n; best_area = area; continue; }       // np.argmax: the first NaN, else the first maximum
        if (best_area != best_area) continue;
        if (area != area || area > best_area) { best = n; best_area = area; }
    }
    const Person &chosen = arena.persons[(size_t)(fr.first_person + best)];
    const double *v = arena.values.data() + chosen.off;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int32_t k = 0; k < n_ids; ++k) {
        const int64_t j = (int64_t)ids[k] * 3;
        const bool keep = v[j + 2] > thr;                             // j[2] > likelihood_threshold
        dst[3 * k + 0] = keep ? v[j + 0] : nan;
        dst[3 * k + 1] = keep ? v[j + 1] : nan;
        dst[3 * k + 2] = keep ? v[j + 2] : nan;
    }
    return true;
}

bool copy_one(const std::string &src, const std::string &dst, std::vector<char> &buf, int &err) {
    if (buf.size() < (1 << 16)) buf.resize(1 << 16);             // before a descriptor is open: resize may throw
    const int in = open(src.c_str(), O_RDONLY | O_CLOEXEC);
    if (in < 0) { err = errno; return false; }
    struct stat st;
    if (fstat(in, &st) != 0) { err = errno; close(in); return false; }
    const int out = open(dst.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (out < 0) { err = errno; close(in); return false; }
    bool ok = true;
    while (ok) {
        const ssize_t r = read(in, buf.data(), buf.size());
        if (r < 0) { err = errno; ok = false; break; }
        if (r == 0) break;
        for (ssize_t w = 0; w < r;) {
            const ssize_t k = write(out, buf.data() + w, (size_t)(r - w));
            if (k < 0) { err = errno; ok = false; break; }
            w += k;
        }
    }
    close(in);
    if (close(out) != 0 && ok) { err = errno; ok = false; }
    if (ok && chmod(dst.c_str(), st.st_mode & 07777) != 0) { err = errno; ok = false; }   // shutil.copymode
    return ok;
}
}  // namespace

extern "C" {

int p2s_json_gather_keypoints(const p2s_json_batch *b, const int32_t *keypoint_ids, int32_t n_ids, int32_t max_persons,
                              const int64_t *file_offsets, int64_t person_stride, int32_t dtype, void *out,
                              int64_t *n_inexact) {
    if (!b || !file_offsets || !out || (n_ids > 0 && !keypoint_ids))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    if (n_ids < 0 || max_persons < 0 || person_stride < 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "negative size");
    if (dtype != P2S_F32 && dtype != P2S_F64) return p2s_set_error(P2S_ERR_INVALID_ARG, "dtype must be P2S_F32 or P2S_F64");
    const int64_t bad = dtype == P2S_F32
        ? gather_keypoints<float>(b, keypoint_ids, n_ids, max_persons, file_offsets, person_stride, (float *)out)
        : gather_keypoints<double>(b, keypoint_ids, n_ids, max_persons, file_offsets, person_stride, (double *)out);
    if (bad < 0) return p2s_set_error(P2S_ERR_OOM, "out of host memory");
    if (n_inexact) *n_inexact = bad;
    return P2S_OK;
}

int p2s_json_gather_people(const p2s_json_batch *b, const int64_t *file_index, const int32_t *person_index,
                           int64_t n_rows, int32_t n_values, int32_t dtype, void *out, int64_t *n_inexact) {
    if (!b || (n_rows > 0 && (!file_index || !person_index || !out)))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    if (n_rows < 0 || n_values < 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "negative size");
    if (dtype != P2S_F32 && dtype != P2S_F64) return p2s_set_error(P2S_ERR_INVALID_ARG, "dtype must be P2S_F32 or P2S_F64");
    for (int64_t r = 0; r < n_rows; ++r) {
        if (file_index[r] < 0 || file_index[r] >= b->n_files)
            return p2s_set_error(P2S_ERR_INVALID_ARG, "row %lld: file index out of range", (long long)r);
        const int32_t cnt = b->files[(size_t)file_index[r]].count;
        if (person_index[r] < 0 || person_index[r] >= cnt)
            return p2s_set_error(P2S_ERR_INVALID_ARG, "row %lld: person index out of range", (long long)r);
    }
    const int64_t bad = dtype == P2S_F32 ? gather_people<float>(b, file_index, person_index, n_rows, n_values, (float *)out)
                                         : gather_people<double>(b, file_index, person_index, n_rows, n_values, (double *)out);
    if (bad < 0) return p2s_set_error(P2S_ERR_OOM, "out of host memory");
    if (n_inexact) *n_inexact = bad;
    return P2S_OK;
}

int p2s_json_gather_largest_person(const p2s_json_batch *b, const int32_t *keypoint_ids, int32_t n_ids,
                                   double likelihood_threshold, double *out) {
    if (!b || (n_ids > 0 && !keypoint_ids) || (b->n_files > 0 && n_ids > 0 && !out))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    if (n_ids < 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "negative size");
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const bool done = parallel_for(b->n_files, host_threads(b->n_threads, 64, b->n_files / 256 + 1), 256, [&](int, int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            double *dst = out + i * (int64_t)n_ids * 3;
            if (!largest_person(b, i, keypoint_ids, n_ids, likelihood_threshold, dst))
                for (int64_t k = 0; k < (int64_t)n_ids * 3; ++k) dst[k] = nan;   // the except branch: all NaN
        }
    });
    return done ? P2S_OK : p2s_set_error(P2S_ERR_OOM, "out of host memory");
}

int p2s_json_person_ids(const p2s_json_batch *b, int64_t *text_off, char *text, int64_t text_capacity, int32_t *file_kind) {
    if (!b || !text_off) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    int64_t at = 0;
    for (int64_t i = 0; i < b->n_files; ++i) {
        const FileRec &fr = b->files[(size_t)i];
        if (file_kind) {
            const int top = (fr.flags >> kFileTopShift) & 7;
            file_kind[i] = fr.count >= 0 ? P2S_JSON_DOC_PEOPLE
                         : fr.count == P2S_JSON_UNREADABLE ? P2S_JSON_DOC_UNREADABLE
                         : top ? P2S_JSON_DOC_LIST + top - 1
                         : (fr.flags & kFilePeopleNull) ? P2S_JSON_DOC_PEOPLE_NULL
                         : (fr.flags & kFilePeopleOther) ? P2S_JSON_DOC_PEOPLE_OTHER : P2S_JSON_DOC_NO_PEOPLE_KEY;
        }
        const Arena &arena = b->arenas[(size_t)fr.thread];
        for (int32_t n = 0; n < fr.count; ++n) {
            const Person &ps = arena.persons[(size_t)(fr.first_person + n)];
            text_off[b->person_base[(size_t)i] + n] = at;
            if (text && ps.id_len && at + ps.id_len <= text_capacity) memcpy(text + at, arena.texts.data() + ps.id_off, (size_t)ps.id_len);
            at += ps.id_len;
        }
    }
    text_off[b->person_base[(size_t)b->n_files]] = at;
    if (text && at > text_capacity) return p2s_set_error(P2S_ERR_INVALID_ARG, "the texts need %lld bytes, %lld given", (long long)at, (long long)text_capacity);
    return P2S_OK;
}

// np.add.reduce over a contiguous float64 vector of fewer than 128 entries: the order of p2s_npsum_small.h
static double numpy_sum_below_128(const double *a, int n) { return p2s_np_sum_below_128<1>(a, n); }

int p2s_json_select_tracked_person(const p2s_json_batch *b, int32_t n_kpts, double conf_threshold, double *out,
                                   int32_t *status, int32_t *detail) {
#pragma clang fp contract(off)                                   // dx*dx + dy*dy as NumPy rounds it: no FMA
    if (!b || (b->n_files > 0 && (!out || !status))) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    if (n_kpts < 1 || n_kpts > 127) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_kpts=%d outside [1, 127]", n_kpts);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int32_t need = 3 * n_kpts;
    const double *prev = nullptr;                                 // the last selection (prev_kp): it lives in an arena
    std::vector<int32_t> cand;
    std::vector<double> dist((size_t)n_kpts);
    auto valid = [&](const double *v, int k) { return v[3 * k + 2] > conf_threshold && !(v[3 * k] != v[3 * k]); };
    for (int64_t i = 0; i < b->n_files; ++i) {
        double *dst = out + i * (int64_t)need;
        for (int32_t k = 0; k < need; ++k) dst[k] = nan;
        if (detail) detail[i] = 0;
        const FileRec &fr = b->files[(size_t)i];
        if (fr.count == P2S_JSON_UNREADABLE) { status[i] = P2S_TRACK_BAD_FILE; continue; }
        if (fr.count == P2S_JSON_NO_PEOPLE_LIST) {
            const bool none = (fr.flags & kFileTopObject) && !(fr.flags & kFilePeopleOther);   // data.get('people', []) is falsy
            status[i] = none ? P2S_TRACK_NO_PEOPLE : P2S_TRACK_BAD_CONTENT;
            continue;
        }
        if (fr.count == 0) { status[i] = P2S_TRACK_NO_PEOPLE; continue; }
        const Arena &arena = b->arenas[(size_t)fr.thread];
        // the reference visits every person before it chooses: the first offending one ends the run
        cand.clear();
        int32_t bad = 0;
        for (int32_t n = 0; n < fr.count && !bad; ++n) {
            const Person &ps = arena.persons[(size_t)(fr.first_person + n)];
            if ((ps.flags & kPersonNotObject) || ps.status == kPersonBadList || ps.status == kPersonNonNumeric || (ps.flags & kPersonHasNull)) {
                bad = P2S_TRACK_BAD_CONTENT;
            } else if (ps.status == kPersonOk && ps.len > need) {
                bad = P2S_TRACK_LONG_LIST;
                if (detail) detail[i] = ps.len;
            } else if (ps.status == kPersonOk && ps.len == need) {
                const double *v = arena.values.data() + ps.off;
                bool any = false;
                for (int k = 0; k < n_kpts && !any; ++k) any = valid(v, k);
                if (any) cand.push_back(n);
            }                                                     // a short or missing list: skipped
        }
        if (bad) { status[i] = bad; continue; }
        if (cand.empty()) { status[i] = P2S_TRACK_NO_CANDIDATE; continue; }
        auto values_of = [&](int32_t n) { return arena.values.data() + arena.persons[(size_t)(fr.first_person + n)].off; };
        int32_t chosen = -1;
        if (cand.size() == 1) {
            chosen = cand[0];
        } else {
            if (prev) {                                           // a selection always has a non-NaN x: never all NaN
                double best = std::numeric_limits<double>::infinity();
                for (int32_t n : cand) {
                    const double *v = values_of(n);
                    int m = 0;
                    for (int k = 0; k < n_kpts; ++k) {
                        if (!valid(v, k) || !valid(prev, k)) continue;
                        const double dx = v[3 * k] - prev[3 * k], dy = v[3 * k + 1] - prev[3 * k + 1];
                        dist[(size_t)m++] = std::sqrt(dx * dx + dy * dy);
                    }
                    if (m == 0) continue;
                    const double mean = numpy_sum_below_128(dist.data(), m) / (double)m;
                    if (mean < best) { best = mean; chosen = n; }  // strictly smaller; NaN and inf never win
                }
            }
            if (chosen < 0) {                                     // the most confidences above the threshold, the first on ties
                int most = -1;
                for (int32_t n : cand) {
                    const double *v = values_of(n);
                    int cnt = 0;
                    for (int k = 0; k < n_kpts; ++k) cnt += v[3 * k + 2] > conf_threshold;
                    if (cnt > most) { most = cnt; chosen = n; }
                }
            }
        }
        const double *v = values_of(chosen);
        for (int32_t k = 0; k < need; ++k) dst[k] = v[k];
        prev = v;
        status[i] = P2S_TRACK_SELECTED;
        if (detail) detail[i] = chosen;
    }
    return P2S_OK;
}

int p2s_copy_files(const char *src_paths, const int64_t *src_offsets, const char *dst_paths, const int64_t *dst_offsets,
                   int64_t n_files, int32_t n_threads, int8_t *ok) {
    if (n_files < 0 || (n_files > 0 && (!src_paths || !src_offsets || !dst_paths || !dst_offsets)))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "bad path table");
    std::atomic<int64_t> first_bad{n_files};
    std::vector<int> errs((size_t)n_files, 0);
    const bool all_run = parallel_for(n_files, host_threads(n_threads, 64, n_files / 64 + 1), 64, [&](int, int64_t lo, int64_t hi) {
        std::vector<char> buf;
        std::string src, dst;
        for (int64_t i = lo; i < hi; ++i) {
            src.assign(src_paths + src_offsets[i], (size_t)(src_offsets[i + 1] - src_offsets[i]));
            dst.assign(dst_paths + dst_offsets[i], (size_t)(dst_offsets[i + 1] - dst_offsets[i]));
            int err = 0;
            const bool done = copy_one(src, dst, buf, err);
            if (ok) ok[i] = done ? 1 : 0;
            if (!done) {
                errs[(size_t)i] = err;
                int64_t cur = first_bad.load();
                while (i < cur && !first_bad.compare_exchange_weak(cur, i)) {}
            }
        }
    });
    if (!all_run) return p2s_set_error(P2S_ERR_OOM, "out of host memory while copying");
    const int64_t bad = first_bad.load();
    if (bad < n_files) {
        const std::string src(src_paths + src_offsets[bad], (size_t)(src_offsets[bad + 1] - src_offsets[bad]));
        return p2s_set_error(P2S_ERR_INVALID_ARG, "copy of %s failed: %s", src.c_str(), strerror(errs[(size_t)bad]));
    }
    return P2S_OK;
}

}  // extern "C"
