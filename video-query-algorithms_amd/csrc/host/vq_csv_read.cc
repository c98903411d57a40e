// The line index of a feature CSV file and the host's value parser (vq_csv_read.h has the rules and what they replace:
// src/api/api_load_records.py:45-58).  Host-only translation unit (no HIP): also built by tests/sanitize_csv/Makefile with
// -fsanitize=address,undefined.
#include "vq_csv_read.h"

#include <locale.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "vq_amd.h"
#include "vq_decimal.h"
#include "vq_host.h"

namespace vq {

namespace {

bool blank(char c) { return c == ' ' || c == '\t'; }
bool digit(char c) { return c >= '0' && c <= '9'; }

// int(row[0]) for what the writer prints and a little more: blanks around an optionally signed run of ASCII digits
bool parse_clip(const char* b, const char* e, int64_t* out) {
    while (b < e && blank(*b)) ++b;
    while (e > b && blank(e[-1])) --e;
    bool neg = false;
    if (b < e && (*b == '+' || *b == '-')) neg = *b++ == '-';
    if (b == e) return false;
    uint64_t v = 0;
    for (; b < e; ++b) {
        if (!digit(*b)) return false;
        if (v > (0x7FFFFFFFFFFFFFFFull - 9) / 10) return false;      // would not fit int64
        v = v * 10 + (uint64_t)(*b - '0');
    }
    *out = neg ? -(int64_t)v : (int64_t)v;
    return true;
}

bool word(const char* b, const char* e, const char* lower) {
    const size_t n = strlen(lower);
    if ((size_t)(e - b) != n) return false;
    for (size_t i = 0; i < n; ++i)
        if ((b[i] | 0x20) != lower[i]) return false;
    return true;
}

}  // namespace

int csv_index(const char* text, int64_t bytes, bool keep, CsvIndex* out, int64_t* n_rows) {
    if (!text || !out || !n_rows || bytes < 0) return host_fail(VQ_E_INVALID, "NULL argument");
    *out = CsvIndex();
    *n_rows = 0;
    if (bytes == 0) return host_fail(VQ_E_INVALID, "line 1: the file is empty (no header line)");
    const char* const end = text + bytes;
    const char* p = text;
    // the header: one line, split by the caller
    for (; p < end && *p != '\n'; ++p) {
        if (*p == '"') return host_fail(VQ_E_UNSUPPORTED, "line 1: a '\"' in the header: quoted CSV is read by tsn/feature_csv.read_features only");
        if (*p == '\r' && !(p + 1 < end && p[1] == '\n')) return host_fail(VQ_E_INVALID, "line 1: a carriage return without a line feed");
    }
    out->header_bytes = csv_line_end(text, p < end ? p + 1 : p) - text;
    if (p < end) ++p;
    int64_t line = 1, rows = 0;
    while (p < end) {
        ++line;
        const char* const start = p;
        const char* first_end = nullptr;          // end of the clip number
        int64_t commas = 0;
        for (; p < end && *p != '\n'; ++p) {
            const unsigned char c = (unsigned char)*p;
            if (c > ',' && c < 0x80) continue;      // digits, letters, '.', '-': nothing to do ('+' is below ',': it takes the slow way)
            if (c == ',') {
                if (!commas) first_end = p;
                ++commas;
            } else if (c == '"') {
                return host_fail(VQ_E_UNSUPPORTED, "line %lld field %lld: a '\"': quoted CSV is read by tsn/feature_csv.read_features only",
                                 (long long)line, (long long)commas);
            } else if (c == '\r') {
                if (!(p + 1 < end && p[1] == '\n'))
                    return host_fail(VQ_E_INVALID, "line %lld field %lld: a carriage return without a line feed", (long long)line, (long long)commas);
            } else if (c >= 0x80 || c == 0) {
                return host_fail(VQ_E_INVALID, "line %lld field %lld: byte 0x%02x in a data row", (long long)line, (long long)commas, c);
            }
        }
        const char* const stop = p < end ? p + 1 : p;     // past the line feed, if there is one
        const char* const le = csv_line_end(start, stop);
        if (le == start) return host_fail(VQ_E_INVALID, "line %lld: an empty data line (the reference's row[0] raises there)", (long long)line);
        if (!first_end) first_end = le;
        if (rows == 0) {
            if (commas < 1) return host_fail(VQ_E_INVALID, "line %lld: a row without a value field", (long long)line);
            if (commas > 0x7FFFFFFF) return host_fail(VQ_E_INVALID, "line %lld: too many fields", (long long)line);
            out->dim = (int32_t)commas;
        } else if (commas != out->dim) {
            return host_fail(VQ_E_INVALID, "line %lld: %lld value fields, the first data row has %d", (long long)line, (long long)commas, out->dim);
        }
        int64_t clip = 0;
        if (!parse_clip(start, first_end, &clip))
            return host_fail(VQ_E_INVALID, "line %lld field 0: '%.*s' is not a clip number", (long long)line, (int)(first_end - start > 40 ? 40 : first_end - start), start);
        if (keep) {
            out->line_off.push_back(start - text);
            out->clip.push_back(clip);
        }
        ++rows;
        p = stop;
    }
    if (keep) out->line_off.push_back(bytes);
    *n_rows = rows;
    return VQ_OK;
}

bool csv_field(const char* begin, const char* end, int64_t field, const char** fb, const char** fe) {
    const char* p = begin;
    for (int64_t k = 0; k < field; ++k) {
        p = (const char*)memchr(p, ',', (size_t)(end - p));
        if (!p) return false;
        ++p;
    }
    const char* q = (const char*)memchr(p, ',', (size_t)(end - p));
    *fb = p;
    *fe = q ? q : end;
    return true;
}

int csv_parse_value(const char* b, const char* e, uint64_t* bits) {
    while (b < e && blank(*b)) ++b;
    while (e > b && blank(e[-1])) --e;
    const char* s = b;
    bool neg = false;
    if (s < e && (*s == '+' || *s == '-')) neg = *s++ == '-';
    const uint64_t sign = neg ? 0x8000000000000000ull : 0ull;
    if (word(s, e, "inf") || word(s, e, "infinity")) {
        *bits = sign | 0x7FF0000000000000ull;
        return 0;
    }
    if (word(s, e, "nan")) {
        *bits = sign | 0x7FF8000000000000ull;
        return 0;
    }
    const vq_dec_field f = vq_dec_scan(b, e);            // the grammar, at any digit count
    if (f.status != VQ_DEC_OK) return -1;
    if (vq_dec_to_double(f.w, f.q, f.digits, f.neg, bits) == VQ_DEC_OK) return 0;
    // what the truncated product cannot decide: the C library, in the "C" locale whatever the process has set
    static const locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    const std::string z(b, e);
    char* stop = nullptr;
    const double v = c_locale ? strtod_l(z.c_str(), &stop, c_locale) : strtod(z.c_str(), &stop);
    if (stop != z.c_str() + z.size()) return -1;
    memcpy(bits, &v, 8);
    return 0;
}

}  // namespace vq

extern "C" int vq_csv_index(const char* text, int64_t bytes, int64_t cap_rows, int64_t* header_bytes, int64_t* n_rows, int32_t* dim,
                            int64_t* line_offsets, int64_t* clip_numbers) {
    if (!text || !header_bytes || !n_rows || !dim) return vq::host_fail(VQ_E_INVALID, "NULL argument");
    const bool keep = line_offsets || clip_numbers;
    vq::CsvIndex ix;
    int64_t n = 0;
    const int rc = vq::csv_index(text, bytes, keep, &ix, &n);
    if (rc != VQ_OK) return rc;
    *header_bytes = ix.header_bytes;
    *n_rows = n;
    *dim = ix.dim;
    if (keep) {
        if (n > cap_rows) return vq::host_fail(VQ_E_INVALID, "the file has %lld data rows, the arrays hold %lld", (long long)n, (long long)cap_rows);
        if (line_offsets) memcpy(line_offsets, ix.line_off.data(), (size_t)(n + 1) * 8);
        if (clip_numbers && n) memcpy(clip_numbers, ix.clip.data(), (size_t)n * 8);
    }
    return VQ_OK;
}
