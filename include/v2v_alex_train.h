/*
 * v2v_alex_train.h -- C ABI of LPIPS-AlexNet as a TRAINING loss in libv2v_hip.so (gfx950): the backward to the prediction of the network
 * whose forward is v2v_lpips_alex.h.  An extension of v2v_hip.h under the same rules: device pointers, sizes and a stream; a v2v_status
 * comes back and its text is behind v2v_last_error(); no entry point allocates or synchronises; arguments are validated before any HIP
 * call.  (A header of its own, as v2v_lpips_alex.h is: that header's export list is pinned name by name.)
 *
 * The gradient goes to the prediction only; backbone and linear layers are frozen.  Everything is float32 NHWC except the compare step,
 * which works per pixel in float64 and rounds once.  No float atomics and no split-K: every output element is summed in one fixed order,
 * so two calls agree bit for bit and an image's result does not depend on how many images share a launch.
 *
 * Compare backward: f0 (pred), f1 (target) float32 [n][HW][C] (C 64, 192, 256 or 384), w float32 [C], ddist float32 [n] -> dz [n][HW][C],
 *   the gradient of  ddist[i] * mean_pixels sum_c w_c (f0_c / n0 - f1_c / n1)^2  with respect to f0.  Per pixel in float64:
 *   r0 = sqrt(sum f0^2), n0 = r0 + 1e-10 (n1 likewise), g_c = 2 w_c (f0_c / n0 - f1_c / n1) ddist / HW,
 *   dz_c = g_c / n0 - f0_c (sum_k g_k f0_k) / (r0 n0^2); the second term is 0 where r0 == 0 (autograd gives NaN there).  relu_mask != 0:
 *   dz_c = 0 where f0_c is not > 0.  dz is written, never added to: a tap's gradient reaches the layer below through `dtap`.
 * Convolution input gradient: ks x ks (5 or 3), stride 1, pad ks / 2.  dy float32 [n][H][W][Cout], Cout a multiple of 32;
 *   weight   float32 [ks * ks * Cout][Cin]: weight[(ky * ks + kx) * Cout + co][ci] = w[co][ci][ks - 1 - ky][ks - 1 - kx], Cin a multiple of 64
 *   dtap     float32 [n][H][W][Cin] or NULL: added to the sum
 *   mask     float32 [n][H][W][Cin] or NULL: the post-ReLU activation that fed the convolution; dx = 0 where it is not > 0
 *   dx       float32 [n][H][W][Cin]
 * Max-pool backward: 3x3 / stride 2, floor mode.  x float32 [n][H][W][C] (the pool's input, C a multiple of 4), dy [n][OH][OW][C] ->
 *   dx [n][H][W][C]: every pixel gathers dy of the windows whose maximum it is (the first maximum in row-major order, as torch), + dtap
 *   ([n][H][W][C] or NULL), then 0 where x is not > 0 when relu_mask != 0.
 * Stem backward: dz float32 [n][OH][OW][64] -> dpred float32 [n][cin][H][W] (contiguous), the transposed 11x11 / stride 4 / pad 2
 *   convolution with weight float32 [3][122][64] (the forward's pack), then per channel in float32: / scale[c], * 2 when normalize,
 *   / divisor when it is not 1.  cin == 1: the three channels are added in channel order before the last two steps.
 *
 * V2V_ERR_SHAPE: n < 0 or > 65535 (compare, stem), H or W < 31 (stem) / < 1 (convolution) / < 3 (pool), cin not 1 or 3, ks not 3 or 5,
 * channel counts not as above, a tensor of 2^31 or more elements.  V2V_ERR_ALIGN: NHWC tensors and weights need 16-byte alignment,
 * everything else 4.  V2V_ERR_PARAM: a divisor that is 0 or not finite.  n == 0 returns V2V_OK without a launch.
 */
#ifndef V2V_ALEX_TRAIN_H
#define V2V_ALEX_TRAIN_H

#include "v2v_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int v2v_alex_train_compare_bwd_hip(const float *f0, const float *f1, const float *w, const float *ddist, int64_t n, int64_t HW, int64_t C, int relu_mask,
                                   float *dz, void *stream);
int v2v_alex_train_conv_dgrad_hip(const float *dy, const float *weight, const float *dtap, const float *mask, int64_t n, int64_t H, int64_t W, int64_t Cin,
                                  int64_t Cout, int ks, float *dx, void *stream);
int v2v_alex_train_pool_bwd_hip(const float *x, const float *dy, const float *dtap, int64_t n, int64_t H, int64_t W, int64_t C, int relu_mask, float *dx,
                                void *stream);
int v2v_alex_train_stem_bwd_hip(const float *dz, const float *weight, const float *scale, int64_t n, int64_t cin, int64_t H, int64_t W, float divisor,
                                int normalize, float *dpred, void *stream);

#ifdef __cplusplus
}
#endif
#endif
