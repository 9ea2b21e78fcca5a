/*
 * v2v_nernet.h -- C ABI of NER-Net's learned event voxelisation in libv2v_hip.so (gfx950).  An extension of v2v_hip.h under the
 * same rules: device pointers, sizes and a stream; a v2v_status comes back and its text is behind v2v_last_error(); no entry point
 * allocates or synchronises; arguments are validated before any HIP call.  (A header of its own: the export list of v2v_hip.h is
 * pinned entry by entry by the contract tests of ABI 6.)
 *
 * The layer (model/nernet/representation_modules.py of the reference): every event row (x, y, t, p, b) adds
 * t_n * MLP(t_n - bin) to each of `bins` bins of its pixel, t_n the per-batch normalised time.  Two launches:
 *
 *   v2v_learned_voxel_stats_hip   first / last row and largest t of every (segment, batch id), by integer atomics
 *   v2v_learned_voxel_hip         normalisation, MLP in registers, float32 atomic scatter
 *
 * events      [n, 5] contiguous rows, float32 (V2V_F32) or float64 (V2V_F64)
 * seg_offsets int64 [n_segments + 1] ascending row offsets, device memory: rows [seg[f], seg[f+1]) form grid f with statistics of
 *             their own; NULL with n_segments == 1 means one grid of all rows.  Rows in no segment are ignored.
 * workspace   v2v_learned_voxel_workspace_bytes(n_segments, batch) bytes, 8-byte aligned; written by the statistics call (which
 *             clears it first), read by the fused call.
 * mlp_layers  HOST array, 3..6 entries, first and last 1, hidden widths 1..128  (e.g. {1, 50, 50, 50, 1})
 * mlp_packed  device float32 [v2v_learned_voxel_packed_elems(...)]; with KP = the largest hidden width rounded up to a multiple
 *             of 16 and every gap zero:   w0[KP] b0[KP]  { W[KP][KP] b[KP] } per hidden Linear (row j = weight[j, :])  wL[KP] bL[KP]
 *             (bL[0] is the last bias).
 * slope       LeakyReLU's negative slope; 0 gives ReLU.
 * out         float32 [n_segments, batch, 2*bins, H, W], positive-polarity half first (combined: [n_segments, batch, bins, H, W]);
 *             cleared by the call (a memset on the stream).
 * t_out       optional float32 [n]: the normalised t of every row in a segment (other rows are not written).
 * combined    QuantizationLayer_trail_combined: p * t_n is both the MLP's input and the factor, no polarity term; float32 rows only.
 *
 * Differences from the reference, on purpose: the rows are not modified; an index below -numel, where put_ raises, drops the term.
 */
#ifndef V2V_NERNET_H
#define V2V_NERNET_H

#include "v2v_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t v2v_learned_voxel_packed_elems(const int *mlp_layers, int n_mlp_layers);
int64_t v2v_learned_voxel_workspace_bytes(int64_t n_segments, int64_t batch);
int v2v_learned_voxel_stats_hip(const void *events, int ev_dtype, int64_t n, const int64_t *seg_offsets, int64_t n_segments, int64_t batch,
                                void *workspace, void *stream);
int v2v_learned_voxel_hip(const void *events, int ev_dtype, int64_t n, const int64_t *seg_offsets, int64_t n_segments, int64_t batch, int bins,
                          int64_t H, int64_t W, const float *mlp_packed, const int *mlp_layers, int n_mlp_layers, float slope, int normalize,
                          int combined, const void *workspace, float *out, float *t_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
