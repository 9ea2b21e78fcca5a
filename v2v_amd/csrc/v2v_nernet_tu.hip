// v2v_nernet_tu.hip -- translation unit of NER-Net's learned voxelisation (v2v_nernet.hpp): its kernels and their C entry points
// (include/v2v_nernet.h).
#include "../../include/v2v_nernet.h"
#include "v2v_nernet.hpp"
#include "v2v_status.hpp"

using v2v::aligned;
using v2v::fail;
using v2v::hip_fail;
using v2v::launched;

namespace {

constexpr int64_t kMaxElems = 0x7FFFFFFFLL;

int padded_width(const int *mlp_layers, int n)
{
    int m = 1;
    for (int l = 1; l < n - 1; ++l) m = mlp_layers[l] > m ? mlp_layers[l] : m;
    return (m + 15) / 16 * 16;
}

int mlp_check(const char *who, const int *mlp_layers, int n)
{
    if (!mlp_layers) return fail(V2V_ERR_NULL, "%s: mlp_layers is NULL", who);
    if (n < 3 || n > v2v::kNerMaxLinear + 1) return fail(V2V_ERR_SHAPE, "%s: mlp_layers needs 3 to 6 entries (got %d)", who, n);
    if (mlp_layers[0] != 1 || mlp_layers[n - 1] != 1) return fail(V2V_ERR_SHAPE, "%s: mlp_layers must start and end with 1", who);
    for (int l = 1; l < n - 1; ++l)
        if (mlp_layers[l] < 1 || mlp_layers[l] > v2v::kNerMaxWidth) return fail(V2V_ERR_SHAPE, "%s: hidden widths must be 1..128 (got %d)", who, mlp_layers[l]);
    return V2V_OK;
}

// events, segments and batch, shared by the two launches
int rows_check(const char *who, const void *events, int ev_dtype, int64_t n, int64_t n_segments, int64_t batch, const void *workspace)
{
    if (!events || !workspace) return fail(V2V_ERR_NULL, "%s: events/workspace is NULL", who);
    if (ev_dtype != V2V_F32 && ev_dtype != V2V_F64) return fail(V2V_ERR_DTYPE, "%s: event rows are float32 or float64", who);
    if (n < 0 || n_segments < 1 || batch < 1 || n * 5 > kMaxElems || n_segments * batch > kMaxElems / 3)
        return fail(V2V_ERR_SHAPE, "%s: need n >= 0, n_segments >= 1, batch >= 1, the event tensor below 2^31 elements (got n %lld, %lld segments, batch %lld)", who,
                    (long long)n, (long long)n_segments, (long long)batch);
    return V2V_OK;
}

template <typename T, int KP>
void launch_fused(const v2v::LearnedVoxelArgs &a, const float *prm, hipStream_t s)
{
    hipLaunchKernelGGL((v2v::learned_voxel_kernel<T, KP>), dim3((unsigned)((a.n + v2v::kNerLanes - 1) / v2v::kNerLanes)), dim3(v2v::kNerLanes), 0, s, a,
                       static_cast<const T *>(a.events), prm);
}

template <typename T>
void launch_width(int kp, const v2v::LearnedVoxelArgs &a, const float *prm, hipStream_t s)
{
    switch (kp) {
    case 16: launch_fused<T, 16>(a, prm, s); break;
    case 32: launch_fused<T, 32>(a, prm, s); break;
    case 48: launch_fused<T, 48>(a, prm, s); break;
    case 64: launch_fused<T, 64>(a, prm, s); break;
    case 80: launch_fused<T, 80>(a, prm, s); break;
    case 96: launch_fused<T, 96>(a, prm, s); break;
    case 112: launch_fused<T, 112>(a, prm, s); break;
    default: launch_fused<T, 128>(a, prm, s); break;
    }
}

}  // namespace

extern "C" {

int64_t v2v_learned_voxel_packed_elems(const int *mlp_layers, int n_mlp_layers)
{
    if (const int rc = mlp_check("v2v_learned_voxel_packed_elems", mlp_layers, n_mlp_layers)) return rc;
    const int64_t kp = padded_width(mlp_layers, n_mlp_layers);
    return 4 * kp + (n_mlp_layers - 3) * (kp * kp + kp);
}

int64_t v2v_learned_voxel_workspace_bytes(int64_t n_segments, int64_t batch)
{
    if (n_segments < 1 || batch < 1 || n_segments * batch > kMaxElems / 3)
        return fail(V2V_ERR_SHAPE, "v2v_learned_voxel_workspace_bytes: need n_segments >= 1, batch >= 1 and their product below 2^31 / 3");
    return n_segments * batch * 24;
}

int v2v_learned_voxel_stats_hip(const void *events, int ev_dtype, int64_t n, const int64_t *seg_offsets, int64_t n_segments, int64_t batch, void *workspace,
                                void *stream)
{
    if (const int rc = rows_check("v2v_learned_voxel_stats_hip", events, ev_dtype, n, n_segments, batch, workspace)) return rc;
    if (!seg_offsets && n_segments != 1) return fail(V2V_ERR_NULL, "v2v_learned_voxel_stats_hip: seg_offsets is NULL with more than one segment");
    if (!aligned(events, ev_dtype == V2V_F64 ? 8 : 4) || !aligned(seg_offsets, 8) || !aligned(workspace, 8))
        return fail(V2V_ERR_ALIGN, "v2v_learned_voxel_stats_hip: events need their element's alignment, seg_offsets/workspace 8-byte alignment");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e = hipMemsetAsync(workspace, 0, (size_t)(n_segments * batch * 24), s);
    if (e != hipSuccess) return hip_fail(e, "v2v_learned_voxel_stats_hip: clearing the workspace");
    if (n == 0) return V2V_OK;
    unsigned long long *st = static_cast<unsigned long long *>(workspace);
    const dim3 grid((unsigned)((n + 255) / 256));
    if (ev_dtype == V2V_F64)
        hipLaunchKernelGGL(v2v::learned_voxel_stats_kernel<double>, grid, dim3(256), 0, s, static_cast<const double *>(events), seg_offsets, n_segments, n, (int)batch, st);
    else
        hipLaunchKernelGGL(v2v::learned_voxel_stats_kernel<float>, grid, dim3(256), 0, s, static_cast<const float *>(events), seg_offsets, n_segments, n, (int)batch, st);
    return launched("learned_voxel_stats_kernel launch");
}

int v2v_learned_voxel_hip(const void *events, int ev_dtype, int64_t n, const int64_t *seg_offsets, int64_t n_segments, int64_t batch, int bins, int64_t H,
                          int64_t W, const float *mlp_packed, const int *mlp_layers, int n_mlp_layers, float slope, int normalize, int combined,
                          const void *workspace, float *out, float *t_out, void *stream)
{
    if (const int rc = rows_check("v2v_learned_voxel_hip", events, ev_dtype, n, n_segments, batch, workspace)) return rc;
    if (!mlp_packed || !out) return fail(V2V_ERR_NULL, "v2v_learned_voxel_hip: mlp_packed/out is NULL");
    if (!seg_offsets && n_segments != 1) return fail(V2V_ERR_NULL, "v2v_learned_voxel_hip: seg_offsets is NULL with more than one segment");
    if (const int rc = mlp_check("v2v_learned_voxel_hip", mlp_layers, n_mlp_layers)) return rc;
    if (combined && ev_dtype != V2V_F32)
        return fail(V2V_ERR_DTYPE, "v2v_learned_voxel_hip: the combined layer takes float32 rows only (the reference fails on float64 rows in nn.Linear)");
    if (bins < 1 || (normalize && bins < 2) || H < 1 || W < 1 || bins > 4096 || H > kMaxElems || W > kMaxElems)
        return fail(V2V_ERR_SHAPE, "v2v_learned_voxel_hip: need bins >= 1 (>= 2 with normalize), H, W >= 1 (got %d x %lld x %lld)", bins, (long long)H, (long long)W);
    const int64_t planes = (combined ? 1 : 2) * (int64_t)bins * batch * n_segments;
    if (H * W > kMaxElems / planes) return fail(V2V_ERR_SHAPE, "v2v_learned_voxel_hip: the output must stay below 2^31 elements");
    if (!aligned(events, ev_dtype == V2V_F64 ? 8 : 4) || !aligned(seg_offsets, 8) || !aligned(workspace, 8) || !aligned(mlp_packed, 4) || !aligned(out, 4) ||
        !aligned(t_out, 4))
        return fail(V2V_ERR_ALIGN, "v2v_learned_voxel_hip: events need their element's alignment, seg_offsets/workspace 8-byte, mlp_packed/out/t_out 4-byte alignment");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e = hipMemsetAsync(out, 0, (size_t)(planes * H * W) * sizeof(float), s);
    if (e != hipSuccess) return hip_fail(e, "v2v_learned_voxel_hip: clearing the output");
    if (n == 0) return V2V_OK;
    v2v::LearnedVoxelArgs a{};
    a.events = events;
    a.seg = seg_offsets;
    a.n_seg = n_segments;
    a.n = n;
    a.B = (int)batch;
    a.C = bins;
    a.H = (int)H;
    a.W = (int)W;
    a.normalize = normalize ? 1 : 0;
    a.combined = combined ? 1 : 0;
    a.n_linear = n_mlp_layers - 1;
    for (int l = 0; l < n_mlp_layers; ++l) a.width[l] = mlp_layers[l];
    a.slope = slope;
    a.stats = static_cast<unsigned long long *>(const_cast<void *>(workspace));
    a.out = out;
    a.t_out = t_out;
    const int kp = padded_width(mlp_layers, n_mlp_layers);
    if (ev_dtype == V2V_F64) launch_width<double>(kp, a, mlp_packed, s);
    else launch_width<float>(kp, a, mlp_packed, s);
    return launched("learned_voxel_kernel launch");
}

}  // extern "C"
