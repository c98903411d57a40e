// Reading the reference's feature files (<stream>_<blob>_features.csv, tsn/feature_csv.py) without the interpreter: the line index
// of a file and the host's parser for the fields the device loader (csrc/vq_csv.hip) hands back.  Host-only translation unit
// (no HIP include): also built with -fsanitize=address,undefined by tests/sanitize_csv/Makefile.
//
// The rules are those of the reference's reader (src/api/api_load_records.py:45-58: csv.reader, int(row[0]), float(x) for the rest)
// on the files its writer produces, and NARROWER than Python's where Python is lenient -- what is refused here stays with
// tsn/feature_csv.read_features:
//   - a '"' anywhere in the file: VQ_E_UNSUPPORTED (quoted CSV);
//   - a carriage return that is not followed by a line feed, a byte >= 0x80 in a data row: VQ_E_INVALID;
//   - a clip number is [ \t]*[+-]?digits[ \t]* that fits int64; a value is the fast-path grammar of vq_decimal.h at any digit
//     count, or inf / infinity / nan in any letter case with an optional sign, either one inside optional spaces or tabs.
//     Python's int() and float() also take underscores between digits, non-ASCII digits and other white space: VQ_E_INVALID here.
// Every error names the 1-based line of the file (the header is line 1) and, where it applies, the 0-based field of that line
// (field 0 is the clip number).
#pragma once
#include <cstdint>
#include <vector>

namespace vq {

struct CsvIndex {
    int64_t header_bytes = 0;            // length of the header line without its line end
    int32_t dim = 0;                     // fields after the first in the first data row (0: no data row)
    std::vector<int64_t> line_off;       // [n_rows + 1]: where each data line starts; the last entry is the file's length
    std::vector<int64_t> clip;           // [n_rows]: int(row[0])
};

// One pass over the file.  With `keep` false only the counts are produced (line_off / clip stay empty, *n_rows is the count).
int csv_index(const char* text, int64_t bytes, bool keep, CsvIndex* out, int64_t* n_rows);

// [begin, end) without its line end: LF or CRLF at the end of a data line is not part of its last field.
inline const char* csv_line_end(const char* begin, const char* end) {
    if (end > begin && end[-1] == '\n') --end;
    if (end > begin && end[-1] == '\r') --end;
    return end;
}

// Field `field` (0-based; 0 is the clip number) of the line [begin, end) (line end already cut off): false if the line has fewer fields.
bool csv_field(const char* begin, const char* end, int64_t field, const char** fb, const char** fe);

// The host's parser of one value field: 0 and the double's bits, or -1 (not a number by the rules above).
int csv_parse_value(const char* begin, const char* end, uint64_t* bits);

}  // namespace vq
