/* Batched query rounds: the weight fit and the re-weighting of up to 16 tickets on the data their pass left on the device.
 *
 * Included by vq_amd.h (do not include it on its own: it needs the vq_db handle, the VQ_E_* codes and the VQ_BROUND_* flags declared
 * there and in vq_amd_rounds.h).  Additive to ABI 12: nothing declared in vq_amd.h, vq_amd_rows.h, vq_amd_rounds.h or
 * vq_amd_round_views.h changes its signature or its behaviour.
 *
 * In the reference a revise or finalize round re-fits its weights on the user's verdicts (src/models/hyperparameter.py:29-76:
 * 40 rescorings, a 40 x 31 loss surface) and rescores under the fitted weights (compute_matches.py:77).  A batched round
 * (vq_db_query_round_batch, vq_db_query_round_views) keeps every query's averaged similarities on the device; the two calls here work
 * on THE LAST BATCHED ROUND OF THE HANDLE, OF EITHER KIND, the way vq_db_batch_round_fetch does:
 *
 *   query q's averaged similarities are that round's device copy -- avg [q][N][S] of a whole-database round, the entries
 *   start[q] .. start[q + 1] of a view round; M_q is the number of its rows (N, or the rows of its view) and every row given or
 *   returned here is a position in [0, M_q), as in that round's results.
 *
 * The copy is a SNAPSHOT: later uploads, presence changes and one-query calls do not touch it; the next batched round replaces it.
 * Every call takes the handle's lock once and uses one upload, one synchronisation and one copy back per run of adjacent queries it
 * serves.  Every failure leaves the snapshot usable.
 *
 * THE FIT BLOCK (vq_db_batch_fit_layout gives the byte offsets, every piece 64-byte aligned; Q = n_queries slots, slot q = query q of
 * the round; sum L = n_labels):
 *
 *   in   off[0] w_grid [Q][G][8] f64 (the first S of a row count) | off[1] th_grid [Q][T] f64 | off[2] ballast [Q] f64 |
 *        off[3] L [Q] i64 (0: the query is skipped) | off[4] rows [sum L] i64, query after query | off[5] labels [sum L] f64, likewise
 *   out  off[6] surface [Q][G][T] f64      off[7] = bytes of the block
 *
 * surface[q][g][t] = 0.5 th[q][t] + sum over query q's labels IN ORDER of (heaviside(score - th, 1) - y) * (score - th) * (1 + y * ballast),
 * score = the score of the labelled row under w_grid[q][g]: the raw sums of vq_db_loss_surface (the caller divides by L_q), with that
 * call's fp64 operations in its order, so a cell has its bits on the same averaged similarities -- for ANY L_q (the labels walk
 * through the workgroup's local memory in chunks of 4096; vq_db_loss_surface itself keeps its limit of 4096).  Cells of a skipped
 * query are not written.
 *
 * THE RE-WEIGHTING reads and writes the block of the round itself (vq_db_batch_round_layout / vq_db_view_round_layout): for every
 * query in `mask` the weights at off[1] and the band at off[2] go up, its scores are recomputed on the device under them (the bits
 * of vq_db_rescore on the same avg), with VQ_BROUND_SELECT it is partitioned again (the rules of vq_db_select, exact on those scores;
 * near_argmax = the first row of the largest near score), and its scores (VQ_BROUND_SCORES), result and prefixes come back.  Entries of
 * queries outside the mask stay as they are, in the host block and on the device: vq_db_batch_round_fetch and
 * vq_db_batch_scores_devptr then serve the new lists and scores of the masked queries and the round's own of the others.
 *
 * ERRORS: VQ_E_STATE -- no batched round on the handle, or a query that round did not have (a slot with L_q > 0, a mask bit);
 * VQ_E_INVALID -- a row outside [0, M_q), G or T outside [1, 64], L_q < 0 or sum L != n_labels, a block that is too short, an unknown
 * flag, an empty mask, a NULL argument.  All of them are checked on the host before anything is launched.
 *
 * OUT OF SCOPE: picking and refining the minimum (vq_db_batch_round_update, vq_amd_round_update.h, chains these two calls around it
 * on the device); sharded databases (one handle only: a row-sharded database fits
 * through vq_db_batch_round_grid, vq_amd_round_grid.h, and sums on the host). */
#ifndef VQ_AMD_ROUND_FIT_H
#define VQ_AMD_ROUND_FIT_H

#ifdef __cplusplus
extern "C" {
#endif

/* off[8] as described above (hyperparameter.py:20-21: the two grids of a fit).  n_queries outside [1, 16], n_grid or n_thresholds
 * outside [1, 64], n_labels < 0 or a NULL argument: VQ_E_INVALID. */
int vq_db_batch_fit_layout(vq_db* db, int32_t n_queries, int32_t n_grid, int32_t n_thresholds, int64_t n_labels, int64_t* off);
/* hyperparameter.py:57-64 for every slot with L_q > 0 in ONE launch: the block's inputs go up in one copy, the loss surfaces of the
 * slots served come back (adjacent slots in one copy), one synchronisation. */
int vq_db_batch_round_fit(vq_db* db, int32_t n_queries, int32_t n_grid, int32_t n_thresholds, int64_t n_labels, void* block, int64_t block_bytes);
/* compute_matches.py:77 (and ticket.py:311-356 with VQ_BROUND_SELECT) for the queries in `mask` (bit q = query q) under the weights
 * and bands `block` -- laid out like the round's own -- holds for them.  flags: VQ_BROUND_SCORES | VQ_BROUND_SELECT. */
int vq_db_batch_round_rescore(vq_db* db, int32_t mask, void* block, int64_t block_bytes, int32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* VQ_AMD_ROUND_FIT_H */
