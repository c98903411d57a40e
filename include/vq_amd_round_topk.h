/* Batched query rounds: the k best clips of every query of the last batched round, ranked on the device in one call.
 *
 * Included by vq_amd.h (do not include it on its own: it needs the vq_db handle and the VQ_E_* codes declared there).  Additive to
 * ABI 12: nothing declared in vq_amd.h, vq_amd_rows.h, vq_amd_csv.h, vq_amd_rounds.h, vq_amd_round_views.h, vq_amd_round_fit.h or
 * vq_amd_round_targets.h changes its signature or its behaviour, and the flags of the round calls are what they were.
 *
 * The reference ranks the clips of a round by a stable descending sort of their scores (src/models/ticket.py:266, the report).
 * vq_db_topk does that for the handle's one-query scores; the scores of a batched round (vq_db_query_round_batch,
 * vq_db_query_round_views, and vq_db_batch_round_rescore behind them) sit in the round's own device block, and the call here ranks
 * them there, for every query at once: one upload (the k's), one synchronisation, one copy back, a launch count that depends neither
 * on the number of queries nor on k, and no sort on the host.  It works on the snapshot of the LAST batched round of the handle, of
 * either kind, as vq_db_batch_round_fetch and vq_db_batch_round_fit do -- whether or not that round copied its scores back.
 *
 * THE BLOCK (page-locked, vq_host_alloc; vq_db_batch_topk_layout gives the byte offsets, every piece 64-byte aligned; Q = n_queries):
 *
 *   in   off[0] k     [Q] i64: how many clips of query q; 0: the query is skipped
 *   out  off[1] count [Q] i64
 *        off[2] rows  [Q][k_max] i64
 *        off[3] vals  [Q][k_max] f64
 *   off[4] = bytes of the block.  off[5] = the largest k_max the call accepts: 4096, so that one workgroup orders a query's survivors
 *   as (key, position) pairs in its local memory.  off[] has 6 entries.
 *
 * PER QUERY (slot q is query q of the round) with k_q > 0: M_q = the entries the round scored for it (N for a whole-database round or
 * a -1 view, else the rows of its view).  count_q = min(k_q, the non-NaN scores among them).  rows[q][:count_q] are POSITIONS in
 * [0, M_q), as in every other result of that round: descending by score, ties by ascending position, -0 and +0 tie, NaN excluded --
 * the rules of vq_db_topk.  vals are the snapshot's scores at those positions, bit for bit.  After vq_db_batch_round_rescore a
 * re-weighted query is ranked under its NEW scores, the others under the round's own.  M_q = 0: count 0.  The entries of a skipped
 * slot are not written; what lies behind count_q in a served slot is unspecified.
 *
 * A piece of at most 16 384 entries whose min(k_q, M_q) is at most 1 024 is ranked by one workgroup in one launch (all such pieces of
 * the call together); a longer piece, or a larger k, takes eight histogram passes, a stable compaction and a sort launch.
 *
 * ERRORS, all found on the host before anything is launched; every failure leaves the snapshot usable.  VQ_E_STATE: no batched round
 * on the handle, or k_q > 0 for a slot the round did not have.  VQ_E_INVALID: a NULL argument; n_queries outside [1, 16]; k_max
 * outside [1, off[5]]; a k_q outside [0, k_max]; a block shorter than off[4].
 *
 * STATE: the call takes the handle's lock once.  It leaves the round's snapshot alone -- scores, avg, n_e, results, the full lists
 * and their counts: vq_db_batch_round_fetch, vq_db_batch_round_fit and vq_db_batch_round_rescore behave afterwards as if it had not
 * run -- and the one-query state of the handle: query, avg, scores, the lists of vq_db_select, the scratch of vq_db_topk, the view
 * in use.  Its own scratch is allocated by the first call, grows on demand and is freed by vq_db_destroy.
 *
 * OUT OF SCOPE: sharded databases; k above off[5] (vq_db_topk, or the scores themselves); ranking inside the pass's own launch. */
#ifndef VQ_AMD_ROUND_TOPK_H
#define VQ_AMD_ROUND_TOPK_H

#ifdef __cplusplus
extern "C" {
#endif

/* off[6] as described above, for ranking up to k_max clips (ticket.py:266: the rows of the report, best score first) of each of
 * n_queries queries.  n_queries outside [1, 16], k_max outside [1, 4096] or a NULL argument: VQ_E_INVALID, before the handle is read. */
int vq_db_batch_topk_layout(vq_db* db, int32_t n_queries, int64_t k_max, int64_t* off);
/* ticket.py:266 (the stable descending sort: best score first, equal scores in position order) for every query of the last batched
 * round with k_q > 0, on the scores that round left on the device. */
int vq_db_batch_round_topk(vq_db* db, int32_t n_queries, int64_t k_max, void* block, int64_t block_bytes);

#ifdef __cplusplus
}
#endif
#endif /* VQ_AMD_ROUND_TOPK_H */
