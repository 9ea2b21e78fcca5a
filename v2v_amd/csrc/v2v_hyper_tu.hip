// v2v_hyper_tu.hip -- translation unit of HyperE2VID's dynamic decoder (v2v_hyper.hpp), inference: its kernels and their C entry points
// (include/v2v_hip.h).
#define V2V_HYPER_KERNELS
#include "../../include/v2v_hip.h"
#include "v2v_hyper.hpp"
#include "v2v_launch.hpp"
#include "v2v_status.hpp"

using v2v::aligned;
using v2v::fail;
using v2v::hip_fail;
using v2v::launched;

extern "C" {

int v2v_hyper_context_hip(const float *events, int64_t stride_b, int64_t stride_c, int64_t stride_h, int64_t stride_w, const float *prev, int64_t B,
                          int64_t C, int64_t H, int64_t W, void *dst, void *stream)
{
    if (!events || !prev || !dst) return fail(V2V_ERR_NULL, "v2v_hyper_context_hip: events/prev/dst is NULL");
    if (B < 1 || C < 1 || C > 7 || H < 4 || W < 4 || H % 4 != 0 || W % 4 != 0 || B * H * W > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "need B >= 1, 1 <= C <= 7, H and W multiples of 4, B*H*W < 2^31");
    if (!aligned(dst, 16) || !aligned(events, 4) || !aligned(prev, 4)) return fail(V2V_ERR_ALIGN, "dst needs 16-byte alignment");
    const int64_t n = B * (H / 4) * (W / 4);
    hipLaunchKernelGGL(v2v::hyper_context_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), events, stride_b, stride_c,
                       stride_h, stride_w, prev, static_cast<uint16_t *>(dst), (int)B, (int)C, (int)H, (int)W);
    return launched("hyper_context_kernel launch");
}

int v2v_hyper_context_conv_hip(const void *x8, const float *weight, const float *bias, int64_t B, int64_t h, int64_t w, int64_t Cin, void *out, void *stream)
{
    if (!x8 || !weight || !bias || !out) return fail(V2V_ERR_NULL, "v2v_hyper_context_conv_hip: x8/weight/bias/out is NULL");
    if (B < 1 || h < 1 || w < 1 || Cin < 1 || Cin > 8 || B * h * w * 32 > 0x7FFFFFFFLL) return fail(V2V_ERR_SHAPE, "need B,h,w >= 1, 1 <= Cin <= 8, output below 2^31 elements");
    if (out == x8) return fail(V2V_ERR_PARAM, "out must not alias x8 (neighbouring pixels read it)");
    if (!aligned(x8, 16) || !aligned(out, 16) || !aligned(weight, 4) || !aligned(bias, 4)) return fail(V2V_ERR_ALIGN, "x8/out need 16-byte alignment");
    const int64_t n = B * h * w * 4;
    hipLaunchKernelGGL(v2v::hyper_context_conv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(x8), weight, bias, static_cast<uint16_t *>(out), (int)B, (int)h, (int)w, (int)Cin);
    return launched("hyper_context_conv_kernel launch");
}

int v2v_tanh_bf16_hip(const void *x, int64_t n, void *out, void *stream)
{
    if (!x || !out) return fail(V2V_ERR_NULL, "v2v_tanh_bf16_hip: x/out is NULL");
    if (n < 8 || n % 8 != 0 || n > 0x7FFFFFFFLL) return fail(V2V_ERR_SHAPE, "need n a multiple of 8 below 2^31");
    if (!aligned(x, 16) || !aligned(out, 16)) return fail(V2V_ERR_ALIGN, "x/out need 16-byte alignment");
    const int64_t n8 = n / 8;
    hipLaunchKernelGGL(v2v::hyper_tanh_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(x), static_cast<uint16_t *>(out), n8);
    return launched("hyper_tanh_kernel launch");
}

int v2v_hyper_atoms_hip(const void *coeff, const float *bases, int64_t M, float *atoms, void *stream)
{
    if (!coeff || !bases || !atoms) return fail(V2V_ERR_NULL, "v2v_hyper_atoms_hip: coeff/bases/atoms is NULL");
    if (M < 1 || M * v2v::kHyAtomElems > 0x7FFFFFFFLL) return fail(V2V_ERR_SHAPE, "need M >= 1 and M * 150 < 2^31");
    if (!aligned(coeff, 2) || !aligned(bases, 4) || !aligned(atoms, 4)) return fail(V2V_ERR_ALIGN, "bases/atoms need 4-byte alignment");
    hipLaunchKernelGGL(v2v::hyper_atoms_kernel, dim3((unsigned)((M * v2v::kHyAtoms + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(coeff), bases, atoms, M);
    return launched("hyper_atoms_kernel launch");
}

int64_t v2v_hyper_dynconv_packed_elems(int64_t Cin, int64_t Cout, int atoms, int ks)
{
    return (Cin == v2v::kHyCin && Cout == v2v::kHyCout && atoms == v2v::kHyAtoms && ks == 5) ? Cin * Cout * atoms : -1;
}

int v2v_hyper_dynconv_pack_weights_hip(const float *weight, int64_t Cin, int64_t Cout, int atoms, void *packed, void *stream)
{
    if (!weight || !packed) return fail(V2V_ERR_NULL, "v2v_hyper_dynconv_pack_weights_hip: weight/packed is NULL");
    if (v2v_hyper_dynconv_packed_elems(Cin, Cout, atoms, 5) < 0) return fail(V2V_ERR_SHAPE, "the dynamic convolution takes Cin 256, Cout 128, 6 atoms");
    if (!aligned(weight, 4) || !aligned(packed, 16)) return fail(V2V_ERR_ALIGN, "weight needs 4-byte, packed 16-byte alignment");
    hipLaunchKernelGGL(v2v::hyper_dynconv_pack_kernel, dim3(v2v::kHyCout * v2v::kHyCin * v2v::kHyAtoms / 256), dim3(256), 0, static_cast<hipStream_t>(stream), weight,
                       static_cast<uint16_t *>(packed));
    return launched("hyper_dynconv_pack_kernel launch");
}

int v2v_hyper_dynconv_nhwc_hip(const void *x, const float *atoms, const void *packed, const float *bias, int relu, int64_t B, int64_t H, int64_t W,
                               int64_t Cin, int64_t Cout, int n_atoms, int ks, void *out, void *stream)
{
    if (!x || !atoms || !packed || !bias || !out) return fail(V2V_ERR_NULL, "v2v_hyper_dynconv_nhwc_hip: x/atoms/packed/bias/out is NULL");
    if (v2v_hyper_dynconv_packed_elems(Cin, Cout, n_atoms, ks) < 0)
        return fail(V2V_ERR_SHAPE, "the dynamic convolution takes Cin 256, Cout 128, 6 atoms, a 5 x 5 window (got %lld -> %lld, %d atoms, ks %d)",
                    (long long)Cin, (long long)Cout, n_atoms, ks);
    if (B < 1 || H < 1 || W < 1 || B * H * W * Cin > 0x7FFFFFFFLL) return fail(V2V_ERR_SHAPE, "need B,H,W >= 1 and tensors below 2^31 elements");
    if (out == x) return fail(V2V_ERR_PARAM, "out must not alias x (neighbouring tiles read it)");
    if (!aligned(x, 16) || !aligned(packed, 16) || !aligned(atoms, 8) || !aligned(out, 2) || !aligned(bias, 4))
        return fail(V2V_ERR_ALIGN, "x/packed need 16-byte, atoms 8-byte alignment");
    static std::atomic<bool> raised[64];                                          // 147 KB of dynamic LDS
    const hipError_t e = v2v::ensure_dynamic_lds(reinterpret_cast<const void *>(&v2v::hyper_dynconv_kernel), v2v::kHyLdsBytes, raised);
    if (e != hipSuccess) return hip_fail(e, "hyper_dynconv_kernel launch");
    const int64_t tiles = B * ((H + v2v::kHyTH - 1) / v2v::kHyTH) * ((W + v2v::kHyTW - 1) / v2v::kHyTW);
    hipLaunchKernelGGL(v2v::hyper_dynconv_kernel, dim3((unsigned)tiles), dim3(512), v2v::kHyLdsBytes, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(x), atoms, static_cast<const uint16_t *>(packed), bias, static_cast<uint16_t *>(out), (int)B, (int)H, (int)W,
                       relu ? 1 : 0);
    return launched("hyper_dynconv_kernel launch");
}

}  // extern "C"
