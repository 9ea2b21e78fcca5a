// v2v_hyper_tu.hip -- translation unit of HyperE2VID's dynamic decoder (v2v_hyper.hpp): launchers.
#define V2V_HYPER_KERNELS
#include "v2v_hyper.hpp"
#include "v2v_launch.hpp"

namespace v2v {

hipError_t launch_hyper_context(const float *ev, int64_t sb, int64_t sc, int64_t sh, int64_t sw, const float *prev, uint16_t *dst, int B, int C, int H, int W,
                                hipStream_t s)
{
    const int64_t n = (int64_t)B * (H / 4) * (W / 4);
    hipLaunchKernelGGL(hyper_context_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ev, sb, sc, sh, sw, prev, dst, B, C, H, W);
    return hipGetLastError();
}

hipError_t launch_hyper_context_conv(const uint16_t *x8, const float *w, const float *bias, uint16_t *out, int B, int h, int wd, int Cin, hipStream_t s)
{
    const int64_t n = (int64_t)B * h * wd * 4;
    hipLaunchKernelGGL(hyper_context_conv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x8, w, bias, out, B, h, wd, Cin);
    return hipGetLastError();
}

hipError_t launch_hyper_tanh(const uint16_t *x, uint16_t *out, int64_t n8, hipStream_t s)
{
    hipLaunchKernelGGL(hyper_tanh_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, x, out, n8);
    return hipGetLastError();
}

hipError_t launch_hyper_atoms(const uint16_t *coeff, const float *bases, float *atoms, int64_t M, hipStream_t s)
{
    hipLaunchKernelGGL(hyper_atoms_kernel, dim3((unsigned)((M * kHyAtoms + 255) / 256)), dim3(256), 0, s, coeff, bases, atoms, M);
    return hipGetLastError();
}

hipError_t launch_hyper_dynconv_pack(const float *w, uint16_t *wp, hipStream_t s)
{
    hipLaunchKernelGGL(hyper_dynconv_pack_kernel, dim3(kHyCout * kHyCin * kHyAtoms / 256), dim3(256), 0, s, w, wp);
    return hipGetLastError();
}

hipError_t launch_hyper_dynconv(const uint16_t *x, const float *atoms, const uint16_t *wp, const float *bias, uint16_t *out, int B, int H, int W, int relu,
                                hipStream_t s)
{
    static std::atomic<bool> raised[64];                                          // 147 KB of dynamic LDS
    const hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(&hyper_dynconv_kernel), kHyLdsBytes, raised);
    if (e != hipSuccess) return e;
    const int64_t tiles = (int64_t)B * ((H + kHyTH - 1) / kHyTH) * ((W + kHyTW - 1) / kHyTW);
    hipLaunchKernelGGL(hyper_dynconv_kernel, dim3((unsigned)tiles), dim3(512), kHyLdsBytes, s, x, atoms, wp, bias, out, B, H, W, relu);
    return hipGetLastError();
}

}  // namespace v2v
