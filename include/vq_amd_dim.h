/* Feature databases of any vector length: a logical length d on rows stored at a zero-padded pitch D.
 *
 * Included by vq_amd.h (do not include it on its own).  Additive to ABI 12 WITHOUT A NEW ENTRY POINT: two flag bits that
 * vq_db_create takes OR-ed into its `dtype` argument.  Without them nothing declared in vq_amd.h changes its behaviour, and a handle
 * made without them runs the kernels, the launches and the bits it ran before (D % 4 != 0 stays VQ_E_INVALID).
 *
 * The reference multiplies whatever vectors `hyperparameters.feature_name` selects (ticket.py:151, np.dot(target_feature,
 * candidate_feature)): 1024 pooled activations, or the 101 class scores of `fc-action`.  A lane of the scans loads four elements,
 * so a plain handle wants D % 4 == 0.  A handle made with VQ_DIM_PADDED has two lengths:
 *
 *   d   the logical length, what the caller's data has: the `D` argument of vq_db_create, any d >= 1;
 *   D   the stored pitch: d rounded up to a multiple of 4.  vq_db_shape answers D.
 *
 * The pads d .. D - 1 of every stored vector are +0.0 -- the whole block is cleared at creation, vq_db_upload and vq_db_load_csv
 * write d values per vector and zero pads -- and the caller keeps the pads of every query +0.0 as well.  A dot over D is then the
 * dot over d exactly (fma(0, 0, p) == p), so everything that reads features works on the pitch, unchanged: the scans (stored
 * D = 1024 -- d = 1021 .. 1024 -- runs the fast kernels and may be tiled), vq_db_set_query_from_row, the Gram matrices of
 * vq_db_bootstrap_target, vq_db_read_rows, row views and the presence mask.
 *
 * On such a handle:
 *   vq_db_upload     takes UNPADDED rows, [nrows][S][E][d] in the database's dtype.  They go up in bounded chunks through a staging
 *                    block on the device, a kernel writes them at pitch D with +0.0 pads into their rows or (a tiled database) their
 *                    tiles: no padded copy is made on the host.  (d == D: the plain upload.)
 *   vq_db_load_csv   compares the file's field count with d and stores at pitch D.
 *   vq_db_generate   fills whole vectors: VQ_E_UNSUPPORTED when d != D.
 *   EVERY OTHER ENTRY POINT KEEPS SPEAKING THE STORED PITCH: vq_db_read_rows, vq_db_set_query, vq_db_set_query_from_row,
 *   vq_db_bootstrap_target, vq_db_round_layout / vq_db_query_round, vq_db_scan_batch and vq_db_adopt_device take and return
 *   vectors of D elements.
 *
 * OUT OF SCOPE: the batched 16-query rounds (they need D in {256, 512, 768, 1024}: stored D = 1024 qualifies, a short database takes
 * one-query rounds); a tiled layout below D = 1024; stored D of 132 .. 1020 keeps the generic scan kernel. */
#ifndef VQ_AMD_DIM_H
#define VQ_AMD_DIM_H

/* vq_db_create(n, S, E, d, dtype | VQ_DIM_PADDED, device, out): `d` is the logical length (any d >= 1), the block is allocated at
 * the pitch (d + 3) / 4 * 4 and cleared to +0.0. */
#define VQ_DIM_PADDED 256
/* ... | VQ_DIM_SHORT_ROWS (implies VQ_DIM_PADDED): stored D <= 128 scans with the short-row kernel -- a wave works on 64 / L clips at
 * once, L = the smallest power of two >= D / 4 lanes per clip, the query in LDS -- instead of the generic one (a wave per vector).
 * The two kernels sum a dot in different orders: they agree to rounding (<= 1e-12 on O(1) similarities), not bit for bit.
 * VQ_SCAN_SHORT=0|1 (vq_amd.h, environment) forces one or the other on every flagged handle of the process. */
#define VQ_DIM_SHORT_ROWS 512

#endif /* VQ_AMD_DIM_H */
