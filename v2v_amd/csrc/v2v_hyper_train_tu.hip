// v2v_hyper_train_tu.hip -- translation unit of the dynamic decoder's BACKWARD (the training kernels of v2v_hyper.hpp) and its C entry points
// (include/v2v_hip.h).
#define V2V_HYPER_TRAIN_KERNELS
#include "../../include/v2v_hip.h"
#include "v2v_hyper.hpp"
#include "v2v_launch.hpp"
#include "v2v_status.hpp"

using v2v::aligned;
using v2v::fail;
using v2v::launched;

namespace {

bool dyn_shape(int64_t B, int64_t H, int64_t W) { return B >= 1 && H >= 1 && W >= 1 && B * H * W * v2v::kHyFCols <= 0x7FFFFFFFLL * 4; }

int64_t dyn_tiles(int64_t B, int64_t H, int64_t W) { return B * ((H + v2v::kHyTH - 1) / v2v::kHyTH) * ((W + v2v::kHyTW - 1) / v2v::kHyTW); }

int dw_splits(int64_t tiles) { return (int)(tiles < 16 ? tiles : 16); }
int db_splits(int64_t M) { return (int)(M < 64 ? M : 64); }

}  // namespace

extern "C" {

const char *v2v_hyper_train_last_error(void) { return v2v_last_error(); }     // deprecated alias, kept for clients linked against ABI 6

int v2v_hyper_dynconv_pack_t_hip(const float *weight, void *packed_t, void *stream)
{
    if (!weight || !packed_t) return fail(V2V_ERR_NULL, "v2v_hyper_dynconv_pack_t_hip: weight/packed_t is NULL");
    if (!aligned(weight, 4) || !aligned(packed_t, 16)) return fail(V2V_ERR_ALIGN, "weight needs 4-byte, packed_t 16-byte alignment");
    hipLaunchKernelGGL(v2v::hyper_dynconv_pack_t_kernel, dim3(v2v::kHyCout * v2v::kHyFCols / 256), dim3(256), 0, static_cast<hipStream_t>(stream), weight,
                       static_cast<uint16_t *>(packed_t));
    return launched("hyper_dynconv_pack_t_kernel launch");
}

int v2v_hyper_dynconv_df_hip(const void *dz, const void *packed_t, int64_t M, void *dF, void *stream)
{
    if (!dz || !packed_t || !dF) return fail(V2V_ERR_NULL, "v2v_hyper_dynconv_df_hip: dz/packed_t/dF is NULL");
    if (M < 1 || M * v2v::kHyFCols > 0x7FFFFFFFLL * 4) return fail(V2V_ERR_SHAPE, "need 1 <= M and M * 1536 below 2^33");
    if (!aligned(dz, 16) || !aligned(packed_t, 16) || !aligned(dF, 16)) return fail(V2V_ERR_ALIGN, "dz/packed_t/dF need 16-byte alignment");
    hipLaunchKernelGGL(v2v::hyper_dynconv_df_kernel, dim3((unsigned)((M + 31) / 32)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(dz), static_cast<const uint16_t *>(packed_t), static_cast<uint16_t *>(dF), M);
    return launched("hyper_dynconv_df_kernel launch");
}

int v2v_hyper_dynconv_datoms_hip(const void *x, const void *dF, int64_t B, int64_t H, int64_t W, float *datoms, void *stream)
{
    if (!x || !dF || !datoms) return fail(V2V_ERR_NULL, "v2v_hyper_dynconv_datoms_hip: x/dF/datoms is NULL");
    if (!dyn_shape(B, H, W)) return fail(V2V_ERR_SHAPE, "need B,H,W >= 1 and B*H*W*1536 below 2^33");
    if (!aligned(x, 16) || !aligned(dF, 16) || !aligned(datoms, 4)) return fail(V2V_ERR_ALIGN, "x/dF need 16-byte alignment");
    static std::atomic<bool> raised[64];
    const hipError_t e = v2v::ensure_dynamic_lds(reinterpret_cast<const void *>(&v2v::hyper_dynconv_datoms_kernel), v2v::kHyDaLdsBytes, raised);
    if (e != hipSuccess) return fail(V2V_ERR_HIP, "hyper_dynconv_datoms_kernel LDS limit: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(v2v::hyper_dynconv_datoms_kernel, dim3((unsigned)dyn_tiles(B, H, W)), dim3(256), v2v::kHyDaLdsBytes, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(x), static_cast<const uint16_t *>(dF), datoms, (int)B, (int)H, (int)W);
    return launched("hyper_dynconv_datoms_kernel launch");
}

int v2v_hyper_dynconv_dx_hip(const float *atoms, const void *dF, int64_t B, int64_t H, int64_t W, void *dx, void *stream)
{
    if (!atoms || !dF || !dx) return fail(V2V_ERR_NULL, "v2v_hyper_dynconv_dx_hip: atoms/dF/dx is NULL");
    if (!dyn_shape(B, H, W)) return fail(V2V_ERR_SHAPE, "need B,H,W >= 1 and B*H*W*1536 below 2^33");
    if (!aligned(atoms, 4) || !aligned(dF, 16) || !aligned(dx, 16)) return fail(V2V_ERR_ALIGN, "dF/dx need 16-byte alignment");
    hipLaunchKernelGGL(v2v::hyper_dynconv_dx_kernel, dim3((unsigned)((B * H * W + 7) / 8)), dim3(256), 0, static_cast<hipStream_t>(stream), atoms,
                       static_cast<const uint16_t *>(dF), static_cast<uint16_t *>(dx), (int)B, (int)H, (int)W);
    return launched("hyper_dynconv_dx_kernel launch");
}

int64_t v2v_hyper_dynconv_wgrad_workspace_bytes(int64_t B, int64_t H, int64_t W)
{
    if (!dyn_shape(B, H, W)) return -1;
    return ((int64_t)dw_splits(dyn_tiles(B, H, W)) * v2v::kHyCout * v2v::kHyFCols + (int64_t)db_splits(B * H * W) * v2v::kHyCout) * 4;
}

int v2v_hyper_dynconv_wgrad_hip(const void *dz, const void *x, const float *atoms, int64_t B, int64_t H, int64_t W, void *workspace, float *dw, float *db,
                                void *stream)
{
    if (!dz || !x || !atoms || !workspace || !dw || !db) return fail(V2V_ERR_NULL, "v2v_hyper_dynconv_wgrad_hip: dz/x/atoms/workspace/dw/db is NULL");
    if (!dyn_shape(B, H, W)) return fail(V2V_ERR_SHAPE, "need B,H,W >= 1 and B*H*W*1536 below 2^33");
    if (!aligned(dz, 16) || !aligned(x, 16) || !aligned(atoms, 4) || !aligned(workspace, 16) || !aligned(dw, 4) || !aligned(db, 4))
        return fail(V2V_ERR_ALIGN, "dz/x/workspace need 16-byte alignment");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    static std::atomic<bool> raised[64];
    const hipError_t e = v2v::ensure_dynamic_lds(reinterpret_cast<const void *>(&v2v::hyper_dynconv_dw_kernel), v2v::kHyWLdsBytes, raised);
    if (e != hipSuccess) return fail(V2V_ERR_HIP, "hyper_dynconv_dw_kernel LDS limit: %s", hipGetErrorString(e));
    const int64_t M = B * H * W, n = (int64_t)v2v::kHyCout * v2v::kHyFCols;
    const int S = dw_splits(dyn_tiles(B, H, W)), Sb = db_splits(M);
    float *const part = static_cast<float *>(workspace), *const part_b = part + (int64_t)S * n;
    hipLaunchKernelGGL(v2v::hyper_dynconv_dw_kernel, dim3(v2v::kHyCin / 16, (unsigned)S), dim3(256), v2v::kHyWLdsBytes, s, static_cast<const uint16_t *>(dz),
                       static_cast<const uint16_t *>(x), atoms, part, (int)B, (int)H, (int)W, S);
    int rc = launched("hyper_dynconv_dw_kernel launch");
    if (rc != V2V_OK) return rc;
    hipLaunchKernelGGL(v2v::hyper_sum_partials_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, dw, n, S);
    rc = launched("hyper_sum_partials_kernel launch");
    if (rc != V2V_OK) return rc;
    hipLaunchKernelGGL(v2v::hyper_bias_partials_kernel, dim3((unsigned)Sb), dim3(128), 0, s, static_cast<const uint16_t *>(dz), part_b, M, Sb);
    rc = launched("hyper_bias_partials_kernel launch");
    if (rc != V2V_OK) return rc;
    hipLaunchKernelGGL(v2v::hyper_sum_partials_kernel, dim3(1), dim3(256), 0, s, part_b, db, (int64_t)v2v::kHyCout, Sb);
    return launched("hyper_sum_partials_kernel launch");
}

int v2v_hyper_bn_stats_hip(const void *z, int64_t M, int64_t Cs, float eps, float *mean, float *var, float *rstd, void *stream)
{
    if (!z || !mean || !var || !rstd) return fail(V2V_ERR_NULL, "v2v_hyper_bn_stats_hip: z/mean/var/rstd is NULL");
    if (M < 1 || Cs < 8 || Cs % 8 != 0 || M * Cs > 0x7FFFFFFFLL) return fail(V2V_ERR_SHAPE, "need M >= 1, Cs a multiple of 8, M * Cs below 2^31");
    if (!aligned(z, 16)) return fail(V2V_ERR_ALIGN, "z needs 16-byte alignment");
    hipLaunchKernelGGL(v2v::hyper_bn_stats_kernel, dim3((unsigned)(Cs / 8)), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint16_t *>(z), M,
                       (int)Cs, eps, mean, var, rstd);
    return launched("hyper_bn_stats_kernel launch");
}

int v2v_hyper_bn_apply_hip(const void *z, const float *mean, const float *rstd, const float *gamma, const float *beta, int64_t M, int64_t Cs, int64_t Cv,
                           int tanh_out, void *out, void *stream)
{
    if (!z || !mean || !rstd || !gamma || !beta || !out) return fail(V2V_ERR_NULL, "v2v_hyper_bn_apply_hip: a pointer is NULL");
    if (M < 1 || Cs < 8 || Cs % 8 != 0 || Cv < 1 || Cv > Cs || M * Cs > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "need M >= 1, Cs a multiple of 8, 1 <= Cv <= Cs, M * Cs below 2^31");
    if (!aligned(z, 16) || !aligned(out, 16)) return fail(V2V_ERR_ALIGN, "z/out need 16-byte alignment");
    hipLaunchKernelGGL(v2v::hyper_bn_apply_kernel, dim3((unsigned)((M * (Cs / 8) + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(z), mean, rstd, gamma, beta, M, (int)Cs, (int)Cv, tanh_out ? 1 : 0, static_cast<uint16_t *>(out));
    return launched("hyper_bn_apply_kernel launch");
}

int v2v_hyper_bn_bwd_hip(const void *dy, int dy_is_f32, const void *z, const float *mean, const float *rstd, const float *gamma, const float *beta, int64_t M,
                         int64_t Cs, int64_t Cv, int tanh_out, float *sums, void *dz, void *stream)
{
    if (!dy || !z || !mean || !rstd || !gamma || !beta || !sums || !dz) return fail(V2V_ERR_NULL, "v2v_hyper_bn_bwd_hip: a pointer is NULL");
    if (M < 1 || Cs < 8 || Cs % 8 != 0 || Cv < 1 || Cv > Cs || M * Cs > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "need M >= 1, Cs a multiple of 8, 1 <= Cv <= Cs, M * Cs below 2^31");
    if (!aligned(dy, 16) || !aligned(z, 16) || !aligned(dz, 16)) return fail(V2V_ERR_ALIGN, "dy/z/dz need 16-byte alignment");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(v2v::hyper_bn_bwd_reduce_kernel, dim3((unsigned)(Cs / 8)), dim3(256), 0, s, dy, dy_is_f32 ? 1 : 0, static_cast<const uint16_t *>(z), mean,
                       rstd, gamma, beta, static_cast<const float *>(nullptr), M, (int)Cs, (int)Cv, tanh_out ? 1 : 0, sums);
    int rc = launched("hyper_bn_bwd_reduce_kernel launch");
    if (rc != V2V_OK) return rc;
    hipLaunchKernelGGL(v2v::hyper_bn_bwd_reduce_kernel, dim3((unsigned)(Cs / 8)), dim3(256), 0, s, dy, dy_is_f32 ? 1 : 0, static_cast<const uint16_t *>(z), mean,
                       rstd, gamma, beta, static_cast<const float *>(sums), M, (int)Cs, (int)Cv, tanh_out ? 1 : 0, sums + 2 * Cs);
    rc = launched("hyper_bn_bwd_reduce_kernel launch (dz sums)");
    if (rc != V2V_OK) return rc;
    hipLaunchKernelGGL(v2v::hyper_bn_bwd_apply_kernel, dim3((unsigned)((M * (Cs / 8) + 255) / 256)), dim3(256), 0, s, dy, dy_is_f32 ? 1 : 0,
                       static_cast<const uint16_t *>(z), mean, rstd, gamma, beta, sums, M, (int)Cs, (int)Cv, tanh_out ? 1 : 0, static_cast<uint16_t *>(dz));
    return launched("hyper_bn_bwd_apply_kernel launch");
}

int v2v_hyper_atoms_bwd_hip(const float *datoms, const void *pre, const float *bases, int64_t M, float *dpre, void *stream)
{
    if (!datoms || !pre || !bases || !dpre) return fail(V2V_ERR_NULL, "v2v_hyper_atoms_bwd_hip: datoms/pre/bases/dpre is NULL");
    if (M < 1 || M * v2v::kHyAtomElems > 0x7FFFFFFFLL) return fail(V2V_ERR_SHAPE, "need M >= 1 and M * 150 < 2^31");
    if (!aligned(datoms, 4) || !aligned(pre, 2) || !aligned(bases, 4) || !aligned(dpre, 4)) return fail(V2V_ERR_ALIGN, "buffers misaligned");
    hipLaunchKernelGGL(v2v::hyper_atoms_bwd_kernel, dim3((unsigned)((M * 8 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), datoms,
                       static_cast<const uint16_t *>(pre), bases, dpre, M);
    return launched("hyper_atoms_bwd_kernel launch");
}

}  // extern "C"
