/* The reference's feature files read without the interpreter: <video>/<split>/<stream>_<blob>_features.csv onto a resident database.
 *
 * Included by vq_amd.h (do not include it on its own: it needs the vq_db handle and the VQ_E_* codes declared there).
 * Additive to ABI 12: nothing declared in vq_amd.h changes.
 *
 * Replaces, for files that are not quoted CSV, the loop of src/api/api_load_records.py:45-58 --
 *
 *     reader = csv.reader(f); header = next(reader)
 *     for row in reader: clip = int(row[0]); feature = [float(x) for x in row[1:]]
 *
 * -- with one pass of the host over the bytes (vq_csv_index: where the lines are, the clip numbers, the field count) and the decimal
 * text converted ON THE DEVICE into the database's own type and layout (vq_db_load_csv).  Every value is the correctly rounded
 * binary64 that float() returns, then rounded ONCE to the database's type (nearest, ties to even).
 *
 * What is read: LF or CRLF line ends; a last line without a line end is a row; an empty data line is VQ_E_INVALID (row[0] raises in
 * the reference); a '"' anywhere is VQ_E_UNSUPPORTED (quoted CSV stays with tsn/feature_csv.read_features); a row whose field count
 * differs from the first data row's is VQ_E_INVALID.  Clip numbers: optionally signed ASCII digits inside optional blanks.  Values:
 * [+-]? digits [. digits*]? ([eE][+-]?digits)? or [+-]? . digits (...), inf / infinity / nan in any letter case with an optional sign,
 * inside optional spaces or tabs.  Underscores, non-ASCII digits and other white space, which Python's int() / float() accept, are
 * VQ_E_INVALID.  Every error names the 1-based line of the file (the header is line 1) and, where it applies, the 0-based field of
 * that line (field 0 is the clip number). */
#ifndef VQ_AMD_CSV_H
#define VQ_AMD_CSV_H

#ifdef __cplusplus
extern "C" {
#endif

/* One pass over a file's bytes.  *header_bytes: length of the header line without its line end (the caller splits it);
 * *n_rows: data rows; *dim: fields after the first in the first data row (0 when there is no data row).
 * line_offsets [n_rows + 1] (byte offset of every data line, then `bytes`) and clip_numbers [n_rows] (int(row[0])) may each be NULL;
 * when one is given, cap_rows says how many rows the arrays hold (VQ_E_INVALID if the file has more: call once with both NULL to
 * count).  Needs no GPU. */
int vq_csv_index(const char* text, int64_t bytes, int64_t cap_rows, int64_t* header_bytes, int64_t* n_rows, int32_t* dim,
                 int64_t* line_offsets, int64_t* clip_numbers);

/* The values of a file (text_host [bytes], header line included) into slot (stream, split) of a database: data row i goes to
 * DATABASE row rows_host[i] (view or no view, like vq_db_upload); -1 skips the row.  VQ_E_INVALID before anything is stored: a row
 * of rows_host outside [-1, N) or named twice, n_rows different from the file's row count, the file's dim different from D -- and
 * everything vq_csv_index refuses.
 * The text goes to the device in chunks of whole lines of at most chunk_bytes (0: 64 MB; a longer line is a chunk of its own) and a
 * workgroup per line converts it; elements are stored in the database's dtype and layout (row-major or tiled).  A line (without
 * its line end) plus its field table must fit the 64 KB of LDS a workgroup may have: lines longer than 65000 - 4 D bytes are
 * VQ_E_UNSUPPORTED (every line the writer can produce fits up to D = 2048: 26 D + 22 bytes).
 * Fields the device does not decide (outside the fast-path grammar, more than 19 significant digits, a rounding the truncated
 * product cannot settle, a value that does not fit a VQ_F16 database) are resolved by the host from the text and patched in;
 * *host_fields (may be NULL) counts them.  A malformed field, or a finite value that binary16 cannot hold (|x| >= 65520, VQ_F16
 * only; VQ_F32 stores inf like numpy's astype), is VQ_E_INVALID naming line and field; the rows the call addressed are then
 * unspecified.  Success invalidates the handle's similarities and scores like vq_db_upload. */
int vq_db_load_csv(vq_db* db, const char* text_host, int64_t bytes, int32_t stream, int32_t split, const int64_t* rows_host,
                   int64_t n_rows, int64_t chunk_bytes, int64_t* host_fields);

#ifdef __cplusplus
}
#endif
#endif /* VQ_AMD_CSV_H */
