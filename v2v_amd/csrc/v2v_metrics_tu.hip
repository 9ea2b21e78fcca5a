// v2v_metrics_tu.hip -- translation unit of the evaluation metrics (v2v_metrics.hpp): its kernels and their C entry points
// (include/v2v_metrics.h).
#include "../../include/v2v_metrics.h"
#include "v2v_metrics.hpp"
#include "v2v_status.hpp"

#include <cmath>

using v2v::aligned;
using v2v::fail;
using v2v::launched;

namespace {

constexpr int64_t kMaxBlocks = 0x7FFFFFFFLL;
constexpr int64_t kMaxSide = 1 << 30;

// tiles per frame of the image kernel, or a status
int64_t image_tiles(const char *who, int64_t T, int64_t H, int64_t W, int64_t *tiles_x, int64_t *tiles_y)
{
    if (T < 0) return fail(V2V_ERR_SHAPE, "%s: T must be >= 0 (got %lld)", who, (long long)T);
    if (H < v2v::kSsimWin || W < v2v::kSsimWin || H > kMaxSide || W > kMaxSide)
        return fail(V2V_ERR_SHAPE, "%s: the 7x7 window needs H >= 7 and W >= 7 (got %lld x %lld)", who, (long long)H, (long long)W);
    *tiles_x = (W - (v2v::kSsimWin - 1) + v2v::kSsimTX - 1) / v2v::kSsimTX;
    *tiles_y = (H - (v2v::kSsimWin - 1) + v2v::kSsimTY - 1) / v2v::kSsimTY;
    if (*tiles_x * *tiles_y > kMaxBlocks / (T > 0 ? T : 1))
        return fail(V2V_ERR_SHAPE, "%s: T * tiles must stay below 2^31 (got T %lld, %lld x %lld)", who, (long long)T, (long long)H, (long long)W);
    return *tiles_x * *tiles_y;
}

// tiles per frame of the flow kernel, or a status
int64_t flow_tiles(const char *who, int64_t T, int64_t H, int64_t W)
{
    if (T < 0) return fail(V2V_ERR_SHAPE, "%s: T must be >= 0 (got %lld)", who, (long long)T);
    if (H < 1 || W < 1 || H >= (1 << 24) || W >= (1 << 24) || H * W >= (1 << 24))
        return fail(V2V_ERR_SHAPE, "%s: need H, W >= 1 and H * W < 2^24, the reference's float32 counts (got %lld x %lld)", who, (long long)H, (long long)W);
    const int64_t tiles = (H * W + v2v::kFlowTile - 1) / v2v::kFlowTile;
    if (tiles > kMaxBlocks / (T > 0 ? T : 1)) return fail(V2V_ERR_SHAPE, "%s: T * tiles must stay below 2^31 (got T %lld)", who, (long long)T);
    return tiles;
}

}  // namespace

extern "C" {

int64_t v2v_image_metrics_workspace_bytes(int64_t T, int64_t H, int64_t W)
{
    int64_t tx, ty;
    const int64_t tiles = image_tiles("v2v_image_metrics_workspace_bytes", T, H, W, &tx, &ty);
    return tiles < 0 ? tiles : T * tiles * v2v::kImgSlots * 8;
}

int v2v_image_metrics_hip(const float *pred, int64_t pred_stride, const float *image, int64_t image_stride, int64_t T, int64_t H, int64_t W, float divisor,
                          double data_range, void *workspace, double *out, double *ssim_map, void *stream)
{
    if (T != 0 && (!pred || !image || !workspace || !out)) return fail(V2V_ERR_NULL, "v2v_image_metrics_hip: pred/image/workspace/out is NULL");
    int64_t tx, ty;
    const int64_t tiles = image_tiles("v2v_image_metrics_hip", T, H, W, &tx, &ty);
    if (tiles < 0) return (int)tiles;
    if (pred_stride < 0 || image_stride < 0) return fail(V2V_ERR_SHAPE, "v2v_image_metrics_hip: frame strides must be >= 0");
    if (!(std::isfinite(divisor) && divisor != 0.0f) || !(std::isfinite(data_range) && data_range > 0.0))
        return fail(V2V_ERR_PARAM, "v2v_image_metrics_hip: divisor must be finite and non-zero, data_range finite and > 0 (got %g, %g)", (double)divisor, data_range);
    if (T == 0) return V2V_OK;
    if (!aligned(pred, 4) || !aligned(image, 4) || !aligned(workspace, 8) || !aligned(out, 8) || !aligned(ssim_map, 8))
        return fail(V2V_ERR_ALIGN, "v2v_image_metrics_hip: pred/image need 4-byte, workspace/out/ssim_map 8-byte alignment");
    v2v::ImageMetricsArgs a{};
    a.pred = pred;
    a.image = image;
    a.pred_stride = pred_stride;
    a.image_stride = image_stride;
    a.H = (int)H;
    a.W = (int)W;
    a.tiles_x = (int)tx;
    a.tiles_y = (int)ty;
    a.divisor = divisor;
    a.c1 = (0.01 * data_range) * (0.01 * data_range);
    a.c2 = (0.03 * data_range) * (0.03 * data_range);
    a.slots = static_cast<double *>(workspace);
    a.map = ssim_map;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(v2v::image_metrics_kernel, dim3((unsigned)(T * tiles)), dim3(v2v::kMetThreads), 0, s, a);
    if (const int rc = launched("image_metrics_kernel launch")) return rc;
    const double wins = (double)((H - (v2v::kSsimWin - 1)) * (W - (v2v::kSsimWin - 1)));
    hipLaunchKernelGGL((v2v::metrics_reduce_kernel<v2v::kImgSlots, 2>), dim3((unsigned)T), dim3(v2v::kMetThreads), 0, s,
                       static_cast<const unsigned long long *>(workspace), tiles, (double)(H * W), wins, out, static_cast<long long *>(nullptr));
    return launched("metrics_reduce_kernel launch");
}

int64_t v2v_flow_metrics_workspace_bytes(int64_t T, int64_t H, int64_t W)
{
    const int64_t tiles = flow_tiles("v2v_flow_metrics_workspace_bytes", T, H, W);
    return tiles < 0 ? tiles : T * tiles * v2v::kFlowSlots * 8;
}

int v2v_flow_metrics_hip(const float *pred, int64_t pred_stride, const float *gt, int64_t gt_stride, const float *events, int64_t ev_stride, int64_t T,
                         int64_t C, int64_t H, int64_t W, void *workspace, int64_t *counts, double *ee_sums, void *stream)
{
    if (T != 0 && (!pred || !gt || !events || !workspace || !counts || !ee_sums))
        return fail(V2V_ERR_NULL, "v2v_flow_metrics_hip: pred/gt/events/workspace/counts/ee_sums is NULL");
    const int64_t tiles = flow_tiles("v2v_flow_metrics_hip", T, H, W);
    if (tiles < 0) return (int)tiles;
    if (C < 1 || C > (1 << 16)) return fail(V2V_ERR_SHAPE, "v2v_flow_metrics_hip: need 1 <= C <= 65536 event channels (got %lld)", (long long)C);
    if (pred_stride < 0 || gt_stride < 0 || ev_stride < 0) return fail(V2V_ERR_SHAPE, "v2v_flow_metrics_hip: frame strides must be >= 0");
    if (T == 0) return V2V_OK;
    if (!aligned(pred, 4) || !aligned(gt, 4) || !aligned(events, 4) || !aligned(workspace, 8) || !aligned(counts, 8) || !aligned(ee_sums, 8))
        return fail(V2V_ERR_ALIGN, "v2v_flow_metrics_hip: pred/gt/events need 4-byte, workspace/counts/ee_sums 8-byte alignment");
    v2v::FlowMetricsArgs a{};
    a.pred = pred;
    a.gt = gt;
    a.events = events;
    a.pred_stride = pred_stride;
    a.gt_stride = gt_stride;
    a.ev_stride = ev_stride;
    a.C = (int)C;
    a.HW = (int)(H * W);
    a.tiles = (int)tiles;
    a.slots = static_cast<unsigned long long *>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(v2v::flow_metrics_kernel, dim3((unsigned)(T * tiles)), dim3(v2v::kMetThreads), 0, s, a);
    if (const int rc = launched("flow_metrics_kernel launch")) return rc;
    hipLaunchKernelGGL((v2v::metrics_reduce_kernel<v2v::kFlowSlots, 2>), dim3((unsigned)T), dim3(v2v::kMetThreads), 0, s,
                       static_cast<const unsigned long long *>(workspace), tiles, 1.0, 1.0, ee_sums, reinterpret_cast<long long *>(counts));
    return launched("metrics_reduce_kernel launch");
}

}  // extern "C"
