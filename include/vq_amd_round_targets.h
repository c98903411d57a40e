/* Batched query rounds: the bootstrapped targets ("dynamic target adjustment") of up to 16 tickets in one call.
 *
 * Included by vq_amd.h (do not include it on its own: it needs the vq_db handle and the VQ_E_* codes declared there).  Additive to
 * ABI 12: nothing declared in vq_amd.h, vq_amd_rows.h, vq_amd_csv.h, vq_amd_rounds.h, vq_amd_round_views.h or vq_amd_round_fit.h
 * changes its signature or its behaviour.
 *
 * In the reference every revise round re-derives its query vectors from the clips the user has validated (src/models/target_clip.py:
 * 26-73): one closed-form problem per (draw, stream, split) (:161-261), bagging averages several draws of one pool of validated
 * clips (:64-73), partial_update blends with the previous round's target (:75-82).  vq_db_bootstrap_target solves ONE draw per call;
 * the call here solves every draw of every query of a group: one upload, one synchronisation, one copy back, no allocation once the
 * handle's buffers have grown, and the Gram matrix of a POOL is computed once however many draws pick from it.
 *
 * THE BLOCK (vq_db_batch_targets_layout gives the byte offsets, every piece 64-byte aligned; Q = n_queries; S, E, D the handle's):
 *
 *   in   off[0] query  [Q][8] i32: R_q rows in the pool | how many of them are matches (they come first) | B_q draws | mode (0: the
 *                                  mean of the draws, 1: blended with `previous`) | 4 unused
 *        off[1] param  [Q][4] f64: mu | keep | 1 - keep (computed by the caller) | unused
 *        off[2] rows   [n_pool_rows] i64: the pools, query after query -- DATABASE rows, whatever view the handle uses
 *        off[3] draw   [n_draws][2] i32: the draws, query after query -- L positions in the draw | how many of them are matches
 *        off[4] pos    [n_entries] i32: the positions of every draw in its query's pool, draw after draw, matches first, in the row
 *                                  order of the problem (target_clip.py:297-309: the iteration order of the draw's set)
 *        off[5] work   library scratch inside the block (the caller neither fills nor reads it)
 *        off[6] previous [Q][S][E][D] f64: read for the queries of mode 1 (not uploaded when there is none)
 *   out  off[7] status [Q][4] i32: 0 solved, 1 singular system | the first draw that failed | its slot s * E + e | unused
 *        off[8] target [Q][S][E][D] f64 (the last piece: query q's part is what off[0] of a round block takes)
 *   off[9] = bytes of the block.  off[10] = the largest draw (rows) whose two systems are solved in the workgroup's local memory;
 *   longer draws solve in a scratch area in device memory, with the same operations.  off[] has 11 entries.
 *
 * PER QUERY: for each draw b and slot (s, e), w_b = the target vq_db_bootstrap_target gives on the draw's rows (valid = the draw's
 * matches, invalid = the rest, the query's mu), bit for bit.  target = (((w_0 + w_1) + w_2) + ...) / B_q (numpy's mean over axis 0;
 * one draw: w_0 itself); mode 1: target = keep * target + (1 - keep) * previous, each product rounded, then the sum.  A singular
 * system (the pivot test of vq_db_bootstrap_target) sets the query's status; its target is not computed and its entries of the
 * target piece hold no result.  The other queries are solved and the call returns VQ_OK.
 *
 * The handle's one-query state (query, similarities, scores, selection), the snapshot of the last batched round and the view in use
 * are left alone.  All three storage types; both layouts of an fp32 database.
 *
 * ERRORS, all VQ_E_INVALID and all found on the host before anything is launched: a NULL argument; Q outside [1, 16]; a row outside
 * [0, N); a pool without a match or of more than 256 rows; B_q outside [1, 64]; a draw without a match, with a position outside its
 * pool (a match position among the non-matches or the other way round), or with a position twice; an unknown mode; counts that do
 * not add up to n_pool_rows, n_draws, n_entries; a block that is too short.
 *
 * OUT OF SCOPE: rows handed over from the host (vq_bootstrap_targets); sharded databases; drawing on the device; leaving the targets
 * on the device for the pass that follows. */
#ifndef VQ_AMD_ROUND_TARGETS_H
#define VQ_AMD_ROUND_TARGETS_H

#ifdef __cplusplus
extern "C" {
#endif

/* off[11] as described above, for the pools, draws and positions of one group (target_clip.py:26-73: the validated clips of a round
 * and the draws of its adjustment mode).  n_queries outside [1, 16], n_pool_rows outside [n_queries, 256 n_queries], n_draws outside
 * [n_queries, 64 n_queries], n_entries outside [n_draws, 256 n_draws] or a NULL argument: VQ_E_INVALID, before the handle is read. */
int vq_db_batch_targets_layout(vq_db* db, int32_t n_queries, int64_t n_pool_rows, int32_t n_draws, int64_t n_entries, int64_t* off);
/* target_clip.py:161-261 for every (draw, stream, split) of the group, target_clip.py:64-73 (the mean of a query's draws) and
 * target_clip.py:75-82 (the blend) in ONE call: a Gram matrix per (pool, slot), the two solves of each draw on its sub-matrix, then
 * the rows combined, averaged and blended in one kernel. */
int vq_db_batch_targets(vq_db* db, int32_t n_queries, int64_t n_pool_rows, int32_t n_draws, int64_t n_entries, void* block, int64_t block_bytes);

#ifdef __cplusplus
}
#endif
#endif /* VQ_AMD_ROUND_TARGETS_H */
