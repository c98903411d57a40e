// Stand-alone driver of the feature-CSV reader's host code, built with -fsanitize=address,undefined (tests/sanitize_csv/Makefile)
// and run as a program by tests/test_csv_decimal_host.py and tests/test_csv_index_host.py.
//
// (fields / csvfields / index / parse take any number of files; index and parse print "file <k>" before each answer)
//   csv_driver fields <file>      one field per line of <file>: the shared header's conversion (csrc/vq_decimal.h) against glibc strtod
//   csv_driver csvfields <csv>    the same over every value field of a feature file (through the indexer)
//   csv_driver probe <field>...   per field: what the shared header says, and what the host's parser returns
//   csv_driver convert <hex>...   per binary64 bit pattern: the binary32 / binary16 storage conversions
//   csv_driver index <csv>        the indexer's answer
//   csv_driver parse <csv>        index + every value the way the loader decides it (shared header first, host parser for the rest)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vq_amd.h"
#include "vq_csv_read.h"
#include "vq_decimal.h"
#include "vq_host.h"

namespace vq {
std::string& last_error_ref() {
    static thread_local std::string s;
    return s;
}
}  // namespace vq

namespace {

bool read_file(const char* path, std::vector<char>* out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    char buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out->insert(out->end(), buf, buf + k);
    fclose(f);
    return true;
}

struct Tally {
    long long fields = 0, decided = 0, undecided = 0, ask_host = 0, mismatches = 0;
    void field(const char* b, const char* e) {
        ++fields;
        uint64_t bits = 0;
        // an exact-size heap copy: a read outside [b, e) is a sanitizer finding
        std::vector<char> exact(b, e);
        const int st = vq_dec_parse(exact.data(), exact.data() + exact.size(), &bits);
        if (st == VQ_DEC_ASK_HOST) {
            ++ask_host;
            return;
        }
        if (st == VQ_DEC_UNDECIDED) {
            ++undecided;
            return;
        }
        ++decided;
        const std::string z(b, e);
        const double want = strtod(z.c_str(), nullptr);
        uint64_t wb;
        memcpy(&wb, &want, 8);
        if (wb != bits) {
            if (++mismatches <= 10) fprintf(stderr, "MISMATCH %s: header %016" PRIx64 " strtod %016" PRIx64 "\n", z.c_str(), bits, wb);
        }
    }
    void print() const {
        printf("fields %lld decided %lld undecided %lld ask_host %lld mismatches %lld\n", fields, decided, undecided, ask_host, mismatches);
    }
};

// the value the loader ends up with: 0 and bits (*host = 1 when the host parser supplied it), or -1
int loader_value(const char* b, const char* e, uint64_t* bits, int* host) {
    std::vector<char> exact(b, e);
    *host = 0;
    if (vq_dec_parse(exact.data(), exact.data() + exact.size(), bits) == VQ_DEC_OK) return 0;
    *host = 1;
    return vq::csv_parse_value(exact.data(), exact.data() + exact.size(), bits);
}

int one_file(const std::string& mode, const char* path, Tally* tally) {
    Tally& t = *tally;
    std::vector<char> raw;
    if (!read_file(path, &raw)) return 3;
    // an exact-size heap block: the indexer reading one byte past the file is a sanitizer finding
    char* text = (char*)malloc(raw.size() ? raw.size() : 1);
    if (!raw.empty()) memcpy(text, raw.data(), raw.size());
    const int64_t bytes = (int64_t)raw.size();
    int status = 0;
    if (mode == "fields") {
        const char* p = text;
        const char* end = text + bytes;
        while (p < end) {
            const char* q = (const char*)memchr(p, '\n', (size_t)(end - p));
            if (!q) q = end;
            t.field(p, q);
            p = q < end ? q + 1 : q;
        }
        free(text);
        return 0;
    }
    vq::CsvIndex ix;
    int64_t n = 0, n_counted = 0;
    const int rc = vq::csv_index(text, bytes, true, &ix, &n);
    if (rc == VQ_OK) {                                           // the C entry point, counting only, must agree
        int64_t hb = 0;
        int32_t dim = 0;
        const int rc2 = vq_csv_index(text, bytes, 0, &hb, &n_counted, &dim, nullptr, nullptr);
        if (rc2 != VQ_OK || hb != ix.header_bytes || n_counted != n || dim != ix.dim) {
            printf("inconsistent\n");
            free(text);
            return 4;
        }
    }
    if (rc != VQ_OK) {
        printf("error %d %s\n", rc, vq::last_error_ref().c_str());
    } else if (mode == "index") {
        printf("ok header_bytes %lld rows %lld dim %d\n", (long long)ix.header_bytes, (long long)n, ix.dim);
        for (int64_t i = 0; i < n; ++i) printf("%lld %lld\n", (long long)ix.clip[(size_t)i], (long long)ix.line_off[(size_t)i]);
        printf("end %lld\n", (long long)ix.line_off[(size_t)n]);
    } else {
        long long host = 0;
        std::string out;
        char buf[32];
        bool refused = false;
        for (int64_t i = 0; i < n && status == 0 && !refused; ++i) {
            const char* lb = text + ix.line_off[(size_t)i];
            const char* le = vq::csv_line_end(lb, text + ix.line_off[(size_t)i + 1]);
            for (int k = 1; k <= ix.dim; ++k) {
                const char *fb, *fe;
                if (!vq::csv_field(lb, le, k, &fb, &fe)) {
                    printf("inconsistent\n");
                    status = 4;
                    break;
                }
                if (mode == "csvfields") {
                    t.field(fb, fe);
                    continue;
                }
                uint64_t bits = 0;
                int h = 0;
                if (loader_value(fb, fe, &bits, &h) != 0) {      // a refusal is an answer, not a failure of the driver
                    printf("error %d line %lld field %d: not a number\n", VQ_E_INVALID, (long long)i + 2, k);
                    refused = true;
                    break;
                }
                host += h;
                snprintf(buf, sizeof buf, "%016" PRIx64 "%c", bits, k == ix.dim ? '\n' : ' ');
                out += buf;
            }
        }
        if (mode == "parse" && status == 0 && !refused) {
            printf("ok header_bytes %lld rows %lld dim %d host_fields %lld\n", (long long)ix.header_bytes, (long long)n, ix.dim, host);
            for (int64_t i = 0; i < n; ++i) printf("%lld%c", (long long)ix.clip[(size_t)i], i + 1 == n ? '\n' : ' ');
            if (n == 0) printf("\n");
            fputs(out.c_str(), stdout);
        }
    }
    free(text);
    return status;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "fields" || mode == "csvfields" || mode == "index" || mode == "parse") {
        Tally t;                                                 // fields / csvfields: over all the files named
        for (int fi = 2; fi < argc; ++fi) {
            if (mode == "index" || mode == "parse") printf("file %d\n", fi - 2);
            const int status = one_file(mode, argv[fi], &t);
            if (status) return status;
        }
        if (mode == "fields" || mode == "csvfields") t.print();
        return 0;
    }
    if (mode == "probe") {
        for (int i = 2; i < argc; ++i) {
            const char* b = argv[i];
            const char* e = b + strlen(b);
            std::vector<char> exact(b, e);
            uint64_t bits = 0, hbits = 0;
            const int st = vq_dec_parse(exact.data(), exact.data() + exact.size(), &bits);
            const int hrc = vq::csv_parse_value(exact.data(), exact.data() + exact.size(), &hbits);
            printf("%s %016" PRIx64 " ", st == VQ_DEC_OK ? "ok" : st == VQ_DEC_ASK_HOST ? "ask_host" : "undecided", st == VQ_DEC_OK ? bits : 0);
            if (hrc == 0)
                printf("host %016" PRIx64 "\n", hbits);
            else
                printf("host invalid\n");
        }
        return 0;
    }
    if (mode == "convert") {
        for (int i = 2; i < argc; ++i) {
            const uint64_t d = strtoull(argv[i], nullptr, 16);
            int o32 = 0, o16 = 0;
            const uint32_t f = vq_f64_to_f32_bits(d, &o32);
            const uint16_t h = vq_f64_to_f16_bits(d, &o16);
            printf("%08x %d %04x %d\n", f, o32, h, o16);
        }
        return 0;
    }
    return 2;
}
