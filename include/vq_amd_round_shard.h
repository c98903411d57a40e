/* Batched query rounds: the two calls that let a ROW-SHARDED database run a group's whole weight update as one operation -- the averaged
 * similarities of chosen rows of the last batched round, verbatim, and vq_db_batch_round_update with the labelled and the user rows'
 * averaged similarities travelling WITH the block instead of being read from the snapshot.
 *
 * Included by vq_amd.h (do not include it on its own: it needs the vq_db handle, the VQ_E_* codes, the VQ_BROUND_* flags of
 * vq_amd_rounds.h and VQ_BUPDATE_SURFACE of vq_amd_round_update.h).  Additive to ABI 12: nothing declared in vq_amd.h or in the round
 * headers before this one changes its signature or its behaviour, and no new constant is defined here.
 *
 * A cell of a loss surface (src/models/hyperparameter.py:57-64) is a function of the labelled clips' averaged similarities avg[row][0..S)
 * and of the grid only; the lowest-scoring match a user confirmed (src/models/ticket.py:301-309) is a function of the user rows' avg and
 * of the picked weights.  A rank of a row-sharded database holds only some of those rows, but S doubles per row are all it lacks.  So
 * the ranks exchange those avg rows ONCE, in front of everything (the first call reads them; they are bit for bit the pass's own
 * values), and every rank then runs the SAME chain on identical tables (the second call): surface in label order, pick and refinement,
 * the rescore of its own rows, the band, the partition of its own rows.  The pick is replicated by construction; only per-row results
 * are gathered afterwards.
 *
 * Both calls act on THE LAST BATCHED ROUND OF THE HANDLE, OF EITHER KIND, with the snapshot semantics of vq_amd_round_fit.h: query q's
 * averaged similarities are that round's device copy, M_q is the number of its rows (N, or the rows of its view).
 *
 * THE AVG-ROWS BLOCK (vq_db_batch_avg_rows_layout gives the byte offsets, every piece 64-byte aligned; Q = n_queries slots, slot q =
 * query q of the round; sum L = n_rows; S = the streams of the handle):
 *
 *   in   off[0] L [Q] i64 (0: the slot is skipped) | off[1] rows [sum L] i64, query after query: positions in [0, M_q), a row may repeat
 *   out  off[2] avg_rows [sum L][S] f64, query after query                                     off[3] = bytes of the block
 *
 * avg_rows[l][s] is a verbatim copy of the snapshot's avg at rows[l]: no arithmetic touches it, so a NaN keeps its payload and -0.0
 * its sign.  One upload (the two input pieces are adjacent), one launch, one copy back, one synchronisation; the handle's lock is taken
 * once; the snapshot and the one-query state of the handle are not written (the call stages in the handle's grid scratch).
 *
 * THE GIVEN-TABLES UPDATE BLOCK (vq_db_batch_update_given_layout) is the block of vq_db_batch_update_layout with two pieces changed:
 *
 *   in   off[4]  label_avg [sum L][S] f64, in label order, query after query   (was: rows [sum L] i64)
 *   in   off[12] user_avg [sum U][S] f64, query after query                    (was: user_rows [sum U] i64)
 *
 * labels, grids, ballast, L, second, eps, band_mode, near, U, pick, pick_idx and the surface piece (out only here) are those of
 * vq_amd_round_update.h.  L_q is the number of labels of the WHOLE database for slot q -- the divisor -- whatever part of them this
 * handle holds.  PER SLOT WITH L_q > 0, in this order:
 *   1. the loss surface: the cell of vq_db_batch_round_fit -- score_from_avg of label l's avg under w_grid[g], the terms added in label
 *      order -- computed by the same kernel from label_avg[l] instead of the snapshot's avg at rows[l];
 *   2. the division by (double)L_q, the first minimum and its refinement, as step 2 of vq_db_batch_round_update;
 *   3. the rescore of THIS HANDLE'S OWN rows of query q under the picked weights, as step 3 there;
 *   4. the band, as step 4 there; mode 1: lowest = 1.0 lowered IN ORDER by score_from_avg(user_avg[i], picked weights) -- the value
 *      the rescore gives at that row on the handle that holds it, folded the same way;
 *   5. with VQ_BROUND_SELECT the partition of this handle's rows of query q under that band, into the block of the round.
 * One upload, one synchronisation; what comes back is what vq_db_batch_round_update copies back.  Every failure leaves the snapshot
 * usable.
 *
 * ERRORS, all checked on the host before anything is launched.  vq_db_batch_round_avg_rows refuses what vq_db_batch_round_grid
 * refuses.  VQ_E_STATE: no batched round on the handle, or a slot with L_q > 0 that the round did not have.  VQ_E_INVALID: a NULL
 * argument; n_queries outside [1, 16]; n_rows < 0 (or above 2^32), an L_q < 0, or sum L != n_rows; a row outside [0, M_q); a block
 * that is too short.  vq_db_batch_round_update_given refuses what vq_db_batch_round_update refuses, minus the row checks (there are
 * no rows), and every flag but VQ_BROUND_SCORES | VQ_BROUND_SELECT | VQ_BUPDATE_SURFACE -- VQ_BUPDATE_GIVEN_SURFACE included.
 *
 * OUT OF SCOPE: the sharded forms of vq_db_query_round_views and of vq_db_batch_targets; an exchange of the tables from device to
 * device without the host block; more than 16 queries; a second GPU (the sharded update built on these calls has run with every rank
 * on one card only). */
#ifndef VQ_AMD_ROUND_SHARD_H
#define VQ_AMD_ROUND_SHARD_H

#ifdef __cplusplus
extern "C" {
#endif

/* off[4] as described above, for the averaged similarities (ticket.py:120-170: the mean over the splits present, per stream) of
 * n_rows rows of n_queries queries.  n_queries outside [1, 16], n_rows < 0 or a NULL argument: VQ_E_INVALID. */
int vq_db_batch_avg_rows_layout(vq_db* db, int32_t n_queries, int64_t n_rows, int64_t* off);
/* ticket.py:120-170 restricted to the rows given, as the last batched round left them on the device, for every slot with L_q > 0 in
 * ONE launch: copies, bit for bit. */
int vq_db_batch_round_avg_rows(vq_db* db, int32_t n_queries, int64_t n_rows, void* block, int64_t block_bytes);
/* off[16] as described above (hyperparameter.py:20-21: the two grids of a fit); the pieces of vq_db_batch_update_layout with
 * label_avg and user_avg S doubles per row.  The refusals of vq_db_batch_update_layout. */
int vq_db_batch_update_given_layout(vq_db* db, int32_t n_queries, int32_t n_grid, int32_t n_thresholds, int64_t n_labels, int64_t n_user_rows,
                                    int64_t* off);
/* hyperparameter.py:57-114, compute_matches.py:77-88 and ticket.py:301-356 for every slot with L_q > 0, the labelled and the user
 * rows' averaged similarities given.  round_block: as for vq_db_batch_round_update.  flags: VQ_BROUND_SCORES | VQ_BROUND_SELECT |
 * VQ_BUPDATE_SURFACE. */
int vq_db_batch_round_update_given(vq_db* db, int32_t n_queries, int32_t n_grid, int32_t n_thresholds, int64_t n_labels, int64_t n_user_rows,
                                   void* update_block, int64_t update_bytes, void* round_block, int64_t round_bytes, int32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* VQ_AMD_ROUND_SHARD_H */
