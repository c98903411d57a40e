/* Row views of a resident feature database: search sets that share one handle.
 *
 * Included by vq_amd.h (do not include it on its own: it needs the vq_db handle and the VQ_E_* codes declared there).
 * Additive to ABI 12: nothing declared in vq_amd.h changes its signature or, with no view in use, its behaviour.
 *
 * A ROW VIEW is a strictly ascending list of M rows of the database (0 <= M <= N), kept on the device.  While a view is in use the
 * ONE-QUERY path runs over it as if the database held only those rows, in database order:
 *
 *   vq_db_scan, vq_db_rescore, vq_db_read_similarities, vq_db_read_scores, vq_db_read_scores_at, vq_db_write_avg,
 *   vq_db_scores_grid, vq_db_loss_surface, vq_db_select, vq_db_select_rows, vq_db_select_fetch, vq_db_topk, vq_db_min_score,
 *   vq_db_query_round and the arrays behind vq_db_scores_devptr / vq_db_avg_devptr / vq_db_ne_devptr
 *
 * work over the M POSITIONS of the view: avg / n_e / sims / scores are compact [M]... arrays (entry i belongs to database row
 * rows[i]); every row argument and every row result of those calls is a position in the view; ties in the top-k go by ascending
 * position and the selection keeps view order.  vq_db_round_layout stays sized for N: the arrays of the block hold their first M
 * entries and only those are copied back.  A clip's dot products, ensemble means and score under a view are the full scan's
 * sequence of operations on the same handle: the same bits (row-major: the scan reads only the M clips; tiled: it reads the
 * tiles the view touches, whole, and a clip outside the view stores nothing).  The tile tables of a view are built when it is defined,
 * for every database of a shape that can be tiled (D = 1024, S <= 2, E <= 5) -- float16 databases included, which have VQ_LAYOUT_TILED16
 * -- so a view defined on rows survives vq_db_set_layout.
 *
 * These stay in DATABASE rows, view or no view: vq_db_set_query_from_row, vq_db_bootstrap_target, vq_db_read_rows,
 * vq_db_upload, vq_db_set_present (the presence mask is [N][S][E] and is read by database row).
 *
 * Not under a view: vq_db_scan_batch and vq_allgather_scores return VQ_E_UNSUPPORTED while one is in use (select the whole database
 * first; a view per query of the 16-query pass is vq_db_query_round_views, vq_amd_round_views.h, which does not consult the view in use).
 *
 * M = 0 is legal: scans launch nothing, the selection returns empty lists and near_argmax = -1, vq_db_topk returns *k_out = 0 and
 * vq_db_min_score 1.
 *
 * A handle keeps any number of views resident (a slot is reused after vq_db_rows_drop); switching between defined views uploads
 * nothing.  Switching invalidates the similarities and scores the handle holds (they cover another population): scan again, or
 * put averaged similarities back with vq_db_write_avg.  A view defined on a row-major database keeps working after
 * vq_db_set_layout(VQ_LAYOUT_TILED) and back: both forms of its index are built when it is defined. */
#ifndef VQ_AMD_ROWS_H
#define VQ_AMD_ROWS_H

#ifdef __cplusplus
extern "C" {
#endif

/* rows_host [m]: strictly ascending, every row in [0, N) -- else VQ_E_INVALID (vq_last_error names the entry: out of range, a
 * duplicate, or out of order).  *view_out: the id of the new view (>= 0).  Does not change the view in use. */
int vq_db_rows_define(vq_db* db, const int64_t* rows_host, int64_t m, int32_t* view_out);
/* The view the one-query path runs over from now on; -1 = the whole database.  An id that is not defined: VQ_E_INVALID.
 * Selecting the view already in use does nothing (and keeps the handle's results). */
int vq_db_rows_use(vq_db* db, int32_t view);
/* Frees a view.  The view in use: VQ_E_STATE; an id that is not defined: VQ_E_INVALID. */
int vq_db_rows_drop(vq_db* db, int32_t view);
/* *view = the view in use (-1: none), *m = the clips the one-query path covers now (M, or N).  Either may be NULL. */
int vq_db_rows_active(vq_db* db, int32_t* view, int64_t* m);

#ifdef __cplusplus
}
#endif
#endif /* VQ_AMD_ROWS_H */
