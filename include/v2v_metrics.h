/*
 * v2v_metrics.h -- C ABI of the evaluation metrics in libv2v_hip.so (gfx950).  An extension of v2v_hip.h under the same rules: device
 * pointers, sizes and a stream; a v2v_status comes back and its text is behind v2v_last_error(); no entry point allocates or
 * synchronises; arguments are validated before any HIP call.  (A header of its own, as v2v_nernet.h is: the export list of v2v_hip.h is
 * pinned entry by entry by the contract tests of ABI 6.)
 *
 * The reference's test loop (ModelInterface.compute_metrics, model/train_utils.py; FlowModelInterface.compute_metrics,
 * model/train_flow_utils.py) for all T frames of a sequence in two launches each: a tile kernel writes partial sums into fixed slots of
 * the workspace, a reduction adds the slots of every frame in slot order.  No float atomics: two calls agree bit for bit.
 *
 * Images: every value is divided by `divisor` first (float32 true division; 1 is skipped).
 *   MSE   the difference in float32, squared and added in float64, over all H * W pixels
 *   SSIM  skimage.metrics.structural_similarity's defaults for one channel: 7x7 uniform window, sample covariance, K1 0.01, K2 0.03,
 *         the mean over the (H-6) * (W-6) windows that lie wholly inside the image; all in float64
 * pred, image   float32 [T][H][W], rows contiguous, *_stride elements from frame to frame (>= 0)
 * data_range    skimage's data_range (the reference passes 2), finite and > 0
 * workspace     v2v_image_metrics_workspace_bytes(T, H, W) bytes, 8-byte aligned
 * out           float64 [T][2] = (mse, ssim)
 * ssim_map      optional float64 [T][H-6][W-6]: S of every window
 *
 * Flow: pred, gt float32 [T][2][H][W], events float32 [T][C][H][W], channels H * W apart, *_stride elements from frame to frame.
 *   valid = !(isnan(gt0) | isnan(gt1) | (gt0 == 0 & gt1 == 0)),  sparse = valid & (sum_c |events_c| > 0),
 *   EE = sqrtf(d0 * d0 + d1 * d1) in float32
 * counts        int64 [T][6] = (n_dense, n_sparse, dense EE > 1, dense EE > 3, sparse EE > 1, sparse EE > 3)
 * ee_sums       float64 [T][2] = the sum of EE over the valid and over the sparse pixels
 * workspace     v2v_flow_metrics_workspace_bytes(T, H, W) bytes, 8-byte aligned
 *
 * V2V_ERR_SHAPE: H < 7 or W < 7 (images; skimage raises there too), H * W >= 2^24 (flow: the reference forms its ratios from float32
 * counts), T < 0, C < 1, a negative stride, more than 2^31 - 1 tiles.  T == 0 returns V2V_OK without a launch.
 */
#ifndef V2V_METRICS_H
#define V2V_METRICS_H

#include "v2v_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t v2v_image_metrics_workspace_bytes(int64_t T, int64_t H, int64_t W);
int v2v_image_metrics_hip(const float *pred, int64_t pred_stride, const float *image, int64_t image_stride, int64_t T, int64_t H, int64_t W,
                          float divisor, double data_range, void *workspace, double *out, double *ssim_map, void *stream);
int64_t v2v_flow_metrics_workspace_bytes(int64_t T, int64_t H, int64_t W);
int v2v_flow_metrics_hip(const float *pred, int64_t pred_stride, const float *gt, int64_t gt_stride, const float *events, int64_t ev_stride,
                         int64_t T, int64_t C, int64_t H, int64_t W, void *workspace, int64_t *counts, double *ee_sums, void *stream);

#ifdef __cplusplus
}
#endif
#endif
