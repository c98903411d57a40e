/* Batched query rounds: the whole weight update of up to 16 tickets -- loss surfaces, the pick and its refinement, the rescore, the
 * review bands and the partition -- in ONE call on the data their pass left on the device.
 *
 * Included by vq_amd.h (do not include it on its own: it needs the vq_db handle, the VQ_E_* codes and the VQ_BROUND_* flags declared
 * there and in vq_amd_rounds.h).  Additive to ABI 12: nothing declared in vq_amd.h or in the round headers before this one changes
 * its signature or its behaviour.
 *
 * vq_db_batch_round_fit and vq_db_batch_round_rescore (vq_amd_round_fit.h) leave the step between them to the host: the minimum of
 * every loss surface and its sub-grid refinement (src/models/hyperparameter.py:66-114), and for a finalize ticket the review band
 * that reaches down to the lowest-scoring match the user confirmed (compute_matches.py:78-88, ticket.py:301-316).  The call here
 * chains all of it on the handle's stream, on THE LAST BATCHED ROUND OF THE HANDLE, OF EITHER KIND, with the snapshot semantics of
 * vq_amd_round_fit.h: it takes the handle's lock once, uploads the update block once, synchronises once and copies back only what
 * `flags` ask for.  Every failure leaves the snapshot usable.
 *
 * THE UPDATE BLOCK (vq_db_batch_update_layout gives the byte offsets, every piece 64-byte aligned; Q = n_queries slots, slot q =
 * query q of the round; sum L = n_labels, sum U = n_user_rows).  off[0] .. off[6] are those of vq_db_batch_fit_layout:
 *
 *   in   off[0] w_grid [Q][G][8] f64 | off[1] th_grid [Q][T] f64 | off[2] ballast [Q] f64 | off[3] L [Q] i64 (0: the slot is skipped) |
 *        off[4] rows [sum L] i64 | off[5] labels [sum L] f64
 *   i/o  off[6] surface [Q][G][T] f64: the raw sums of vq_db_batch_round_fit; back with VQ_BUPDATE_SURFACE, UP with
 *        VQ_BUPDATE_GIVEN_SURFACE (the piece travels with the one upload either way)
 *   in   off[7] second [Q] i32: the column of w_grid that carries the grid | off[8] eps [Q] f64 (COMPUTE_EPS) |
 *        off[9] band_mode [Q] i32: 0 = reach is near[q], 1 = reach from the user's confirmed matches | off[10] near [Q] f64 |
 *        off[11] U [Q] i64 | off[12] user_rows [sum U] i64, query after query: positions in the query's piece (mode 1)
 *   out  off[13] pick [Q][8] f64: w_best, threshold (= th_best - eps), lowest (mode 1, else 1.0), band[2] = (threshold, lower), 0, 0, 0
 *        off[14] pick_idx [Q][4] i32: iw, it, state (bit 0: the minimum lies on the rim of the grid, bit 1: the refinement fell back
 *        to the cell), 0                                                                     off[15] = bytes of the block
 *        (the pick and pick_idx rows of a slot with L_q == 0 are UNDEFINED after the call: nothing computes them)
 *
 * PER SLOT WITH L_q > 0, in this order (a slot with L_q == 0 is skipped and stays exactly as the round left it):
 *   1. the loss surface of vq_db_batch_round_fit, unless it is given;
 *   2. every cell divided by (double)L_q, then the FIRST minimum in row-major order, a NaN cell counting as smaller than every number
 *      (numpy.argmin); inside the grid the separable three-point parabola of hyperparameter.py:78-114, fp64, no contraction, squares
 *      as products, min / max as Python's (a NaN vertex stays NaN and never exceeds the tolerance); on the rim the grid values;
 *   3. the scores of vq_db_batch_round_rescore under row iw of w_grid with column `second` replaced by w_best;
 *   4. the band (threshold, threshold - reach (1 - threshold)); mode 1: lowest = 1.0 lowered by every score at user_rows IN ORDER
 *      (v < m ? v : m -- NaN scores are skipped), reach = max(threshold - lowest, 0) / max(1 - threshold, eps);
 *   5. with VQ_BROUND_SELECT the partition of vq_db_batch_round_rescore under that band, into the block of the round.
 *
 * ERRORS, all checked on the host before anything is launched.  VQ_E_STATE: no batched round on the handle, or a slot with L_q > 0
 * that the round did not have.  VQ_E_INVALID: a NULL argument, n_queries outside [1, 16], G or T outside [1, 64], n_labels or
 * n_user_rows < 0, an unknown flag or both surface flags, a block that is too short, L_q or U_q < 0, sums that differ from n_labels
 * (without a given surface) or n_user_rows, and for a slot with L_q > 0: a row or a user row outside [0, M_q), `second` outside
 * [0, S), a band_mode other than 0 and 1.
 *
 * OUT OF SCOPE: sharded databases (one handle only: a row-sharded database runs this update as one operation on the two calls of
 * vq_amd_round_shard.h, which carry the rows' averaged similarities with the block; the given-surface flag alone does not give a
 * finalize member its band), the k best clips
 * (vq_db_batch_round_topk follows this call as it follows the rescore), more than 16 queries. */
#ifndef VQ_AMD_ROUND_UPDATE_H
#define VQ_AMD_ROUND_UPDATE_H

#ifdef __cplusplus
extern "C" {
#endif

#define VQ_BUPDATE_SURFACE 16        /* copy the raw loss surfaces of the slots served back */
#define VQ_BUPDATE_GIVEN_SURFACE 32  /* the raw loss surfaces come with the block: no fit launch; rows and labels are not read */

/* off[16] as described above (hyperparameter.py:20-21: the two grids of a fit).  n_queries outside [1, 16], n_grid or n_thresholds
 * outside [1, 64], n_labels or n_user_rows < 0 or a NULL argument: VQ_E_INVALID. */
int vq_db_batch_update_layout(vq_db* db, int32_t n_queries, int32_t n_grid, int32_t n_thresholds, int64_t n_labels, int64_t n_user_rows, int64_t* off);
/* hyperparameter.py:57-114, compute_matches.py:77-88 and ticket.py:311-356 for every slot with L_q > 0.  round_block: the block of the
 * round itself (vq_db_batch_round_layout / vq_db_view_round_layout), needed with VQ_BROUND_SCORES (the slots' scores come back into
 * it) or VQ_BROUND_SELECT (results and prefixes); entries of other queries stay as they are.  flags: VQ_BROUND_SCORES |
 * VQ_BROUND_SELECT | VQ_BUPDATE_SURFACE | VQ_BUPDATE_GIVEN_SURFACE. */
int vq_db_batch_round_update(vq_db* db, int32_t n_queries, int32_t n_grid, int32_t n_thresholds, int64_t n_labels, int64_t n_user_rows,
                             void* update_block, int64_t update_bytes, void* round_block, int64_t round_bytes, int32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* VQ_AMD_ROUND_UPDATE_H */
