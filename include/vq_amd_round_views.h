/* Batched query rounds with a row view per query: up to 16 tickets, each on its own search set, in ONE read of the UNION of their sets.
 *
 * Included by vq_amd.h (do not include it on its own: it needs the vq_db handle, the VQ_E_* codes and the VQ_BROUND_* flags declared
 * there and in vq_amd_rounds.h).  Additive to ABI 12: nothing declared in vq_amd.h, vq_amd_rows.h or vq_amd_rounds.h changes its
 * signature or its behaviour -- vq_db_query_round_batch and vq_db_scan_batch keep refusing while a view is in use.
 *
 * In the reference every query has a search set (src/models/ticket.py:358-365 fetches the candidates of self.search_set), so tickets
 * whose sets are row views of one resident database (vq_amd_rows.h) meet in a pass here: the pass of vq_db_query_round_batch walks the
 * union U of the queries' views once, and query q is scored (ticket.py:165-180), averaged (ticket.py:155-160) and partitioned
 * (ticket.py:311-356) over ITS view only.  views_host[q] is a defined view id of the handle, or -1 = the whole database; M_q is the
 * number of its rows (N for -1).  If a view is -1, U is the whole database.
 *
 * THE BLOCK (page-locked: vq_host_alloc) is the batched round's block with the per-query pieces concatenated instead of strided by N
 * -- vq_db_view_round_layout gives the byte offsets, every piece 64-byte aligned, and start[q], the first entry of query q's piece
 * (start[Q] = sum M; the entries behind Q repeat it):
 *
 *   in   off[0] t [Q][S][E][D] f64 | off[1] weights [Q][8] f64 (the first S of a row count) | off[2] band [Q][2] f64 (threshold, lower)
 *   out  off[3] n_e [sum M][S] i32 | off[4] avg [sum M][S] f64 | off[5] scores [sum M] f64 | off[6] result [Q][4] i64 (n_match, n_near,
 *        near_argmax, 0) | off[7] match prefix [Q][P] i64 | off[8] near prefix [Q][P] i64
 *        off[9] = bytes of the block, off[10] = P, off[11] = sum M
 *
 * Entry start[q] + i of n_e / avg / scores belongs to position i of query q's view, i.e. to database row rows[i] of that view; every
 * row in a result (the lists, near_argmax) is a POSITION in that query's view, as under vq_amd_rows.h.  M_q = 0 is legal: empty
 * lists, near_argmax = -1; if every view is empty nothing is launched.
 *
 * BITS: a (clip, query) pair's avg and score have the bits vq_db_query_round_batch gives that pair on the same handle and layout with
 * the query in the same slot (the same operands in the same k order through the same matrix-core sequence; where a clip sits in a
 * tile does not enter its output element); the partition is exact on those scores.  Against the one-query round under the view
 * (vq_db_rows_use + vq_db_query_round) they agree to rounding (<= 1e-12), as the batched pass does.
 *
 * PRECONDITIONS, those of vq_db_query_round_batch: 1 <= Q <= 16, D in {256, 512, 768, 1024}, S <= 8; float32, float64 and float16
 * storage, and the tiled layout for float32.  The flags are the VQ_BROUND_* values.
 *
 * STATE: the view in use (vq_db_rows_use) is neither consulted nor changed and the one-query state of the handle is left alone,
 * exactly as vq_db_query_round_batch leaves it.  vq_db_batch_round_fetch and vq_db_batch_round_times serve the last batched round of
 * either kind.  After a view round vq_db_batch_scores_devptr has no [Q][N] array to name: it fails with VQ_E_STATE until the next
 * whole-database pass.  The plan of a round (an inverse map [16][N] int32 and the union list) is built on the device per call, O(N +
 * sum M) work and no host copy of that size; its block is allocated on the first view round and freed by vq_db_destroy.
 *
 * OUT OF SCOPE: a plan cached across calls; sharded databases (one handle only). */
#ifndef VQ_AMD_ROUND_VIEWS_H
#define VQ_AMD_ROUND_VIEWS_H

#ifdef __cplusplus
extern "C" {
#endif

/* off[12] and start[17] as described above (ticket.py:358-365: one search set per query).  n_queries outside [1, 16], a NULL
 * argument, or a view id that is not defined on the handle (vq_last_error names the query): VQ_E_INVALID. */
int vq_db_view_round_layout(vq_db* db, int32_t n_queries, const int32_t* views_host, int64_t* off, int64_t* start);
/* One locked call (ticket.py:120-180, 311-356 for every query): inputs up in one copy, the plan, ONE pass over the union of the views,
 * n_e per query, (VQ_BROUND_SELECT) the Q partitions, ONE synchronisation, and what `flags` asks for comes back.  block_bytes < off[9],
 * an unknown flag bit, n_queries outside [1, 16], a NULL argument or an undefined view id: VQ_E_INVALID. */
int vq_db_query_round_views(vq_db* db, int32_t n_queries, const int32_t* views_host, void* block, int64_t block_bytes, int32_t flags);
/* Of the last view round (ticket.py:358-365: the clips its queries' search sets name together): *n_union = the rows in the union
 * of its views, *n_tiles = the tiles of 16 rows the union touches (what a tiled database read).  Either may be NULL.  VQ_E_STATE
 * without such a round. */
int vq_db_view_round_union(vq_db* db, int64_t* n_union, int64_t* n_tiles);

#ifdef __cplusplus
}
#endif
#endif /* VQ_AMD_ROUND_VIEWS_H */
