/* Batched query rounds: the scores of chosen rows of the last batched round under a grid of weights, for every query in one call.
 *
 * Included by vq_amd.h (do not include it on its own: it needs the vq_db handle and the VQ_E_* codes declared there).  Additive to
 * ABI 12: nothing declared in vq_amd.h, vq_amd_rows.h, vq_amd_csv.h, vq_amd_rounds.h, vq_amd_round_views.h, vq_amd_round_fit.h,
 * vq_amd_round_targets.h or vq_amd_round_topk.h changes its signature or its behaviour.
 *
 * In the reference a weight fit rescores the whole search set under each of 40 candidate weights and reads the labelled clips' scores
 * (src/models/hyperparameter.py:57-58).  vq_db_scores_grid gives those scores for the one-query state of a handle and
 * vq_db_batch_round_fit folds them into a loss surface on the device.  A cell of that surface is the sum of one term per labelled
 * clip IN LABEL ORDER, so a rank of a row-sharded database, which holds only some of the labelled rows, cannot produce a cell's bits
 * from a partial sum: it needs the scores themselves, combines the disjoint pieces of the ranks exactly (x + 0) and adds the terms in
 * label order on the host.  The call here gives those scores on THE LAST BATCHED ROUND OF THE HANDLE, OF EITHER KIND, the way
 * vq_db_batch_round_fit reads it: query q's averaged similarities are that round's device copy, M_q is the number of its rows (N, or
 * the rows of its view) and every row given here is a position in [0, M_q).
 *
 * THE BLOCK (vq_db_batch_grid_layout gives the byte offsets, every piece 64-byte aligned; Q = n_queries slots, slot q = query q of
 * the round; G = n_grid; sum L = n_rows):
 *
 *   in   off[0] w_grid [Q][G][8] f64 (the first S of a row count) | off[1] L [Q] i64 (0: the query is skipped) |
 *        off[2] rows [sum L] i64, query after query
 *   out  off[3] graded f64: per query with L_q > 0 a [G][L_q] piece, query after query      off[4] = bytes of the block
 *
 * graded[q][g][l] = score_from_avg of the snapshot's averaged similarities at rows[l] under w_grid[q][g] -- the bits vq_db_scores_grid
 * gives on the same avg, and, with G = 1 and the weights of the round (or of the vq_db_batch_round_rescore behind it), the bits of
 * that round's own score at that row.  A row may be listed more than once.
 *
 * One upload (the three input pieces are adjacent), one launch (a thread per (q, g, l)), one copy back, one synchronisation; the
 * handle's lock is taken once.  The snapshot -- avg, scores, n_e, results, lists -- and the one-query state of the handle are not
 * written; the call stages in the handle's grid scratch, as vq_db_scores_grid and vq_db_batch_round_fit do.
 *
 * ERRORS, all checked on the host before anything is launched; every failure leaves the snapshot usable.  VQ_E_STATE: no batched
 * round on the handle, or a slot with L_q > 0 that the round did not have.  VQ_E_INVALID: n_queries outside [1, 16]; n_grid outside
 * [1, 64]; n_rows < 0 (or above 2^32), an L_q < 0, or sum L != n_rows; a row outside [0, M_q); a block shorter than off[4]; a NULL argument.
 *
 * OUT OF SCOPE: the sharded forms of vq_db_query_round_views (FeatureDB.query_round_batch_sets) and of vq_db_batch_targets -- a
 * ShardedFeatureDB batches whole-database rounds only; picking the minimum of a loss surface on the device (vq_amd_round_update.h on
 * one handle, vq_amd_round_shard.h for a sharded database, which then needs no grid scores); a second GPU (the sharded rounds built
 * on this call have run with every rank on one card only). */
#ifndef VQ_AMD_ROUND_GRID_H
#define VQ_AMD_ROUND_GRID_H

#ifdef __cplusplus
extern "C" {
#endif

/* off[5] as described above, for the scores of n_rows rows (hyperparameter.py:57-58: the labelled clips under each candidate weight)
 * of n_queries queries under n_grid weights each.  n_queries outside [1, 16], n_grid outside [1, 64], n_rows < 0 or a NULL argument:
 * VQ_E_INVALID, before the handle is read. */
int vq_db_batch_grid_layout(vq_db* db, int32_t n_queries, int32_t n_grid, int64_t n_rows, int64_t* off);
/* hyperparameter.py:57-58 restricted to the rows given, for every slot with L_q > 0 in ONE launch, on the averaged similarities the
 * last batched round left on the device. */
int vq_db_batch_round_grid(vq_db* db, int32_t n_queries, int32_t n_grid, int64_t n_rows, void* block, int64_t block_bytes);

#ifdef __cplusplus
}
#endif
#endif /* VQ_AMD_ROUND_GRID_H */
