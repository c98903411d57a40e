// The direct convolution of the TSN executor as the executor (vq_tsn.hip) sees it: the arguments of a launch, the table of tilings
// and one launcher.  The kernels, their instantiations and the rule for which kernel serves a tiling are in vq_tsn_conv.hip.
#pragma once
#include <cstddef>

#include "vq_tsn_kernels.h"   // FullDiv

// (ConvSeg and ConvArgs are outside namespace vq: ConvArgs is the kernels' parameter type and part of their symbol names)
// Where a group of 32 output columns of a convolution goes.  One convolution may feed several tensors (sibling 1x1
// convolutions of an inception block merged into one GEMM): the table has one entry per 32-column group.
struct ConvSeg {
    float* out_base;     // destination slot + its channel offset - first column of the segment: index with the GEMM column
    int Cs;              // channel stride of the destination slot
    int relu;
};

struct ConvArgs {
    const float* in;
    const ConvSeg* segs; // [ceil(Cout / 32)]
    float* out;
    const float* w;      // [Cout][Kp], k index = (kh*k + kw)*Cin + c, zero padded to Kp
    const float* bias;   // [Cout]
    const float* zeros;  // >= 16 bytes of zeros: where masked-off lanes load from (no branches around loads)
    int H, W, Cs_in, coff_in, Cin;
    int Ho, Wo, Cs_out, coff_out, Cout;
    int k, stride, pad;  // k kernel rows ...
    int kw;              // ... of kw taps each (= k, or 1 when a kernel row is folded into the channel axis, see launch_conv_layer)
    int col_off;         // aligned mode: floats between the 16-byte chunk columns of a staged row (4 = consecutive channels), and
    int c_step;          // floats the channel offset advances per K-step (BK).  The x-major space-to-depth stem stages ROW r of its
                         // four kernel rows in chunk column r instead: col_off = the slot's row pitch, c_step = 4 (launch_conv_layer)
    int M, Kp, relu;
    int out_row0;        // first output row (pixel) of this launch inside the destination slots (sub-batch launches)
    int pool_k, pool_s;  // POOL kernels: the 1x1 convolution reads max over a pool_k x pool_k window (stride pool_s, no padding,
                         // clipped at the image edge) of the H x W source instead of a pixel; Ho x Wo is the pooled size
    int tiles_m, tiles_n;
    unsigned in_bytes, w_bytes;   // extents for the buffer descriptors (out-of-range offsets read as zero)
    int ksplit;          // > 1: the grid is ksplit x tiles; slice ks sums K floats [ks * k_per, (ks + 1) * k_per) only and stores
    int k_per;           // its raw partial sums (zero bias, no ReLU) through segs[ks * seg_stride ..] into a scratch plane;
    int seg_stride;      // splitk_combine_kernel adds the planes in slice order, then bias and ReLU.  Aligned Cin only.
    // conv_igemm_pipe_kernel: the pixel decoding of a workgroup without a division (fill_pixel_walk)
    unsigned m_tiles_n;            // magic_div constant for tiles_n
    vq::FullDiv d_howo, d_wo;      // first pixel of the tile -> (image, row, column) on the scalar unit
    unsigned s_wo, s_ho;           // recip22 constants: the per-lane walk of at most BM pixels from there
};

namespace vq {

// A launch of one instantiation: tiles_m, tiles_n and the pipelined kernel's division constants are filled in a
typedef int (*ConvLaunch)(ConvArgs& a, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop);

// One tiling of the direct kernels: BM x BN x BK on four waves, and the kernels it has (null: none).  The executor reads the entries
// as flags and launches through launch_conv, which knows which of them serves a layer.
struct ConvTile {
    int bm, bn, bk;
    int pipe;                // 0 = plain kernel; 1 = software-pipelined kernel (aligned Cin only); 3 = pool_gemm_kernel (pooled-input 1x1
                             // layers only; bk is its k-group of 8).  2 is taken: vq_tsn_layer_tiles reports the Winograd form with it
    ConvLaunch conv[2];      // plain kernel, aligned / small Cin (also in a pipelined tiling: shapes outside its reciprocal range)
    ConvLaunch piped[2];     // pipelined kernel, aligned / small Cin
    ConvLaunch pooled;       // pooled-input layers: the plain kernel's pooled loader, or pool_gemm_kernel
};

// Candidate tilings.  Every candidate sums each output element's K terms in the same order, so the choice never changes a result bit;
// the autotuner and the occupancy heuristic (vq_tsn.hip) both take the first of equals in this order.
extern const ConvTile* const kTiles;   // [kNumTiles]
extern const int kNumTiles;

// The entry of the external form [bm, bn, bk, pipe] of a tiling (vq_tsn_set_tiles, VQ_TSN_TILE); -1: none
int tile_index(int bm, int bn, int bk, int pipe);

// pool_gemm_kernel's LDS for BM pixels of K channels, and whether a pooled-input layer of K channels has a kernel under tiling t
size_t pool_gemm_lds(int bm, int K);
bool pooled_ok(const ConvTile& t, int K);

// Run tiling ti on the arguments a (after launch_conv_layer's row folding; tiles_m, tiles_n and the pipelined kernel's division
// constants are filled here) on `stream`.  ev_start / ev_stop: as for launch_wino_group.  A tiling without a kernel for the layer is
// replaced by one that gives the same bits where there is one; VQ_E_INVALID where there is none.
int launch_conv(int ti, ConvArgs& a, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop);

}  // namespace vq
