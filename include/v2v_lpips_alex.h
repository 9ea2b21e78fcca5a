/*
 * v2v_lpips_alex.h -- C ABI of the LPIPS-AlexNet test metric in libv2v_hip.so (gfx950).  An extension of v2v_hip.h under the same rules:
 * device pointers, sizes and a stream; a v2v_status comes back and its text is behind v2v_last_error(); no entry point allocates or
 * synchronises; arguments are validated before any HIP call.  (A header of its own, as v2v_metrics.h is: the export list of v2v_hip.h is
 * pinned entry by entry by the contract tests of ABI 6.)
 *
 * The network is PerceptualSimilarity/models/networks_basic.py:PNetLin(pnet_type='alex', version='0.1', spatial=False) in eval mode,
 * forward only.  Everything is float32: activations float32 NHWC, weights float32, accumulation float32 on the float32-input matrix-core
 * instruction, whose result is a k-ordered fmaf chain.  There is no split-K: the order in which an output element is summed is fixed, so
 * a frame's result does not depend on how many frames share a launch.  No float atomics: two calls agree bit for bit.
 *
 * Sizes: a side s becomes (s - 7) / 4 + 1 through the stem and (s - 3) / 2 + 1 through a pool (integer division).
 *
 * Stem: frames float32 [n][cin][H][W], cin 1 or 3, channels H * W apart, frame_stride elements from frame to frame (>= 0).  Per value, in
 *   float32 and in this order: x / divisor (a true division; 1 is skipped), 2 x - 1 when normalize, (x - shift[c]) / scale[c] for the three
 *   channels c (a one-channel frame is read three times).  Then the 11x11 / stride 4 / pad 2 convolution to 64 channels, + bias, ReLU; the
 *   padding is zero after the scaling.
 *   weight   float32 [3][122][64]: weight[c][ky * 11 + kx][o] = w[o][c][ky][kx], row 121 of every channel zero
 *   out      float32 [n][OH][OW][64]
 * Convolution: ks x ks (5 or 3), stride 1, pad ks / 2, + bias, ReLU when relu != 0.
 *   x        float32 [n][H][W][Cin], Cin a multiple of 32
 *   weight   float32 [ks * ks * Cin][Cout]: weight[(ky * ks + kx) * Cin + ci][o] = w[o][ci][ky][kx], Cout a multiple of 64
 *   y        float32 [n][H][W][Cout]
 * Max-pool: 3x3 / stride 2, no padding, floor mode.  x float32 [n][H][W][C], C a multiple of 4 -> y [n][(H-3)/2+1][(W-3)/2+1][C].
 * Compare: f0, f1 float32 [n][HW][C] (C 64, 192, 256 or 384), w float32 [C].  Per pixel in float64: nrm = sqrt(sum_c f_c^2) + 1e-10 for
 *   both, sum_c w_c (f0_c / nrm0 - f1_c / nrm1)^2; a pixel whose features are all zero contributes 0.  Tiles of 64 pixels write their sums
 *   into fixed slots of the workspace; a second launch adds an image's slots in slot order and writes taps[i][tap] = sum / HW.
 *   workspace  v2v_lpips_alex_compare_workspace_bytes(n, HW) bytes, 8-byte aligned
 *   taps       float64 [n][5], tap in 0..4
 * Sum: dist[i] = the five taps[i][.] each rounded to float32, added in tap order in float32.
 *
 * V2V_ERR_SHAPE: n < 0, H or W < 31 (stem) / < 1 (convolution) / < 3 (pool), cin not 1 or 3, ks not 3 or 5, Cin / Cout / C not as above,
 * a negative stride, a tensor of 2^31 or more elements, tap outside 0..4.  V2V_ERR_ALIGN: NHWC tensors and weights need 16-byte alignment,
 * workspace and taps 8, everything else 4.  V2V_ERR_PARAM: a divisor that is 0 or not finite.  n == 0 returns V2V_OK without a launch.
 */
#ifndef V2V_LPIPS_ALEX_H
#define V2V_LPIPS_ALEX_H

#include "v2v_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int v2v_lpips_alex_stem_hip(const float *frames, int64_t frame_stride, int64_t n, int64_t cin, int64_t H, int64_t W, float divisor, int normalize,
                            const float *shift, const float *scale, const float *weight, const float *bias, float *out, void *stream);
int v2v_lpips_alex_conv_hip(const float *x, const float *weight, const float *bias, int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int ks,
                            int relu, float *y, void *stream);
int v2v_lpips_alex_pool_hip(const float *x, int64_t n, int64_t H, int64_t W, int64_t C, float *y, void *stream);
int64_t v2v_lpips_alex_compare_workspace_bytes(int64_t n, int64_t HW);
int v2v_lpips_alex_compare_hip(const float *f0, const float *f1, const float *w, int64_t n, int64_t HW, int64_t C, int tap, void *workspace, double *taps,
                               void *stream);
int v2v_lpips_alex_sum_hip(const double *taps, int64_t n, float *dist, void *stream);

#ifdef __cplusplus
}
#endif
#endif
