/* Batched query rounds: up to 16 queries -- 16 tickets -- in ONE read of a resident feature database.
 *
 * Included by vq_amd.h (do not include it on its own: it needs the vq_db handle and the VQ_E_* codes declared there).
 * Additive to ABI 12: nothing declared in vq_amd.h changes its signature or its behaviour.
 *
 * vq_db_query_round (vq_amd.h) is one query's round in one call: scan, scores, review partition, one copy back.  A batched round
 * is the same per query for Q queries that share the pass of vq_db_scan_batch: the database is read once, every query gets
 *
 *   avg [N][S]     the averaged similarities of ticket.py:155-160 (fp64), stored where the pass closes a stream
 *   scores [N]     the scores of vq_db_scan_batch on the same inputs, bit for bit (the pass only gained stores)
 *   the partition  match = {v >= threshold}, near = {lower <= v < threshold}, both in database order, and near_argmax = the first
 *                  row of the largest near score (-1: none) -- the rules of vq_db_select, each query under its OWN (threshold, lower)
 *
 * and n_e [N][S] (int32: the splits present under the handle's effective presence mask, E everywhere without one) is produced once,
 * it does not depend on the query.  The dots run on the fp64 matrix cores, so avg and scores equal the one-query scan's to rounding
 * (<= 1e-12), not bit for bit; everything derived from the batched scores (the partition) is exact on those scores.
 *
 * THE BLOCK (page-locked: vq_host_alloc) -- vq_db_batch_round_layout gives the byte offsets, every piece 64-byte aligned:
 *
 *   in   off[0] t [Q][S][E][D] f64 | off[1] weights [Q][8] f64 (the first S of a row count) | off[2] band [Q][2] f64 (threshold, lower)
 *   out  off[3] n_e [N][S] i32 | off[4] avg [Q][N][S] f64 | off[5] scores [Q][N] f64 | off[6] result [Q][4] i64 (n_match, n_near,
 *        near_argmax, 0) | off[7] match prefix [Q][P] i64 | off[8] near prefix [Q][P] i64
 *        off[9] = bytes of the block, off[10] = P, the prefix length (the off[9] of vq_db_round_layout), off[11] = 0
 *
 * The first min(count, P) rows of each list come back next to the counts; the full lists stay on the device until the next batched
 * round on the handle and vq_db_batch_round_fetch copies those of one query out when a count exceeds P.
 *
 * PRECONDITIONS, those of vq_db_scan_batch: 1 <= Q <= 16, D in {256, 512, 768, 1024}, S <= 8, and the WHOLE database -- with a row
 * view in use (vq_amd_rows.h) the call returns VQ_E_UNSUPPORTED and says so.  float32, float64 and float16 storage, rows and tiled
 * layout (each storage type's own: VQ_LAYOUT_TILED, VQ_LAYOUT_TILED64, VQ_LAYOUT_TILED16 -- on a tiled database of any type the pass
 * gives the bits of the pass on its rows).
 *
 * THE ONE-QUERY STATE of the handle is left alone, as vq_db_scan_batch leaves it: the query, avg, n_e, scores, the selection lists
 * of vq_db_select and the view in use.  The batched buffers are allocated on the first call and freed by vq_db_destroy.  After a
 * batched round vq_db_batch_scores_devptr names ITS scores.
 *
 * A row view per query: vq_db_query_round_views (vq_amd_round_views.h).  The weight fit (a batched vq_db_loss_surface) and the
 * re-weighting of a round's queries on the data it left on the device: vq_amd_round_fit.h.  The k best clips of every query, ranked on
 * the scores the round left on the device: vq_amd_round_topk.h.  OUT OF SCOPE: sharded databases (one handle only); more than 16
 * queries per pass (split the list: a pass costs one read of the database). */
#ifndef VQ_AMD_ROUNDS_H
#define VQ_AMD_ROUNDS_H

#ifdef __cplusplus
extern "C" {
#endif

#define VQ_BROUND_AVG 1      /* copy n_e and avg back */
#define VQ_BROUND_SCORES 2   /* copy the scores back */
#define VQ_BROUND_SELECT 4   /* partition every query under its band; results and prefixes come back */
#define VQ_BROUND_TIMED 8    /* record the events vq_db_batch_round_times reads */

/* off[12] as described above, for n_queries queries.  n_queries outside [1, 16]: VQ_E_INVALID. */
int vq_db_batch_round_layout(vq_db* db, int32_t n_queries, int64_t* off);
/* One locked call: the block's queries, weights and bands go up in one copy, the 16-query pass, n_e, (VQ_BROUND_SELECT) the Q
 * partitions, ONE synchronisation, and what `flags` asks for comes back (adjacent pieces in one copy).  The pass and the scores
 * always run.  block_bytes < off[9] or an unknown flag bit: VQ_E_INVALID; a row view in use: VQ_E_UNSUPPORTED. */
int vq_db_query_round_batch(vq_db* db, int32_t n_queries, void* block, int64_t block_bytes, int32_t flags);
/* The full lists of query `query` of the last batched round (which must have partitioned).  Either pointer may be NULL; a buffer
 * shorter than its count: VQ_E_INVALID; no such round, or a query it did not have: VQ_E_STATE.  Mirrors vq_db_select_fetch. */
int vq_db_batch_round_fetch(vq_db* db, int32_t query, int64_t* match_rows_host, int64_t cap_match, int64_t* near_rows_host, int64_t cap_near);
/* ms[3] of the last round run with VQ_BROUND_TIMED: upload + pass + n_e | selection | copies back (device time between events).
 * VQ_E_STATE without such a round. */
int vq_db_batch_round_times(vq_db* db, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* VQ_AMD_ROUNDS_H */
