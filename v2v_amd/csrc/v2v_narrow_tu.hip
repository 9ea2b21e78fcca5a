// v2v_narrow_tu.hip -- translation unit of the 16-channel layer family (FireNet): the fused ConvGRU step, the fused residual block, the
// 16-output head and their weight packing.  Kernels and layouts in v2v_narrow.hpp.
#define V2V_NARROW_KERNELS
#include "v2v_narrow.hpp"

namespace v2v {

namespace {
unsigned narrow_grid(const NarrowArgs &a) { return (unsigned)((int64_t)a.B * a.tiles_x * a.tiles_y); }
}  // namespace

hipError_t launch_convgru16(const NarrowArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(narrow_two_conv_kernel<0>, dim3(narrow_grid(a)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_resblock16(const NarrowArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(narrow_two_conv_kernel<1>, dim3(narrow_grid(a)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_conv_head16(const NarrowArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(narrow_head_kernel, dim3(narrow_grid(a)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_convgru16_pack(const float *w_u, const float *w_r, const float *w_o, uint16_t *wp, hipStream_t s)
{
    hipLaunchKernelGGL(narrow_pack_kernel, dim3(kGru16Frags * kNarrowFragElems / 256), dim3(256), 0, s, 0, w_u, w_r, w_o, 0, wp);
    return hipGetLastError();
}

hipError_t launch_resblock16_pack(const float *w1, const float *w2, uint16_t *wp, hipStream_t s)
{
    hipLaunchKernelGGL(narrow_pack_kernel, dim3(kRes16Frags * kNarrowFragElems / 256), dim3(256), 0, s, 1, w1, w2, static_cast<const float *>(nullptr), 0, wp);
    return hipGetLastError();
}

hipError_t launch_conv_head16_pack(const float *w, int Cin, uint16_t *wp, hipStream_t s)
{
    hipLaunchKernelGGL(narrow_pack_kernel, dim3(kHead16Frags * kNarrowFragElems / 256), dim3(256), 0, s, 2, w, static_cast<const float *>(nullptr),
                       static_cast<const float *>(nullptr), Cin, wp);
    return hipGetLastError();
}

}  // namespace v2v
