// v2v_convlstm_tu.hip -- translation unit of the fused ConvLSTM step and of the layers that share its kernels'
// header: convolution, head, stem, 1x1, upsampling, layout.  The launchers that choose an instance, then the C entry points
// (include/v2v_hip.h).
#include "../../include/v2v_hip.h"
#include "v2v_convlstm.hpp"
#include "v2v_args.hpp"
#include "v2v_status.hpp"

namespace v2v {

// tile_rows: pixels per workgroup tile (64, 128 or 256); 0 = auto: the largest tile that still gives every CU a workgroup.
// Same box, 8 clips (ms per step; tools/ab_convlstm.sh):        64 px    128 px   256 px
//   64 ch @128^2 / 128 ch @64^2 / 256 ch @32^2 (256^2 input)     0.119/0.100/0.094   0.114/0.096/0.089   0.101/0.083/0.126
//   64 ch @64^2 / 128 ch @32^2 / 256 ch @16^2 (128^2 input)      0.034/0.042/0.071   0.033/0.048/0.080   0.049/0.074/0.127
hipError_t launch_convlstm_step(const ConvLstmArgs &a, int tile_rows, hipStream_t s)
{
    if (tile_rows == 0) {
        const int cus = device_cus();
        const int64_t m = (int64_t)a.B * a.H * a.W, ct = a.C / kClCh;
        tile_rows = (m / 256 * ct >= cus) ? 256 : (m / 128 * ct >= cus) ? 128 : 64;      // (a partial last tile is fine: any B*H*W)
        // when even 64-pixel tiles give a CU at most one workgroup: that workgroup as two K groups (KS = 2; same box, 8 clips:
        // 128 ch @32^2 0.039 -> 0.033 ms, 256 ch @16^2 0.067 -> 0.053 ms; slower where more tiles exist: 0.115 -> 0.144 ms)
        if (tile_rows == 64 && m / 64 * ct <= cus) tile_rows = 65;
    }
    // (round 4, measured and not kept: tiles of ONE wave column -- 32 hidden channels x 4 gates -- so that two workgroups share a CU and
    // one's epilogue runs under the other's main loop: launch_step_t<1, 4, 2, 0, 1, 4>, 128 px x 32 ch, 64 KB: 0.107 / 0.101 / 0.098 ms
    // against 0.088 / 0.078 / 0.095 for the tiles below at 64@128^2 / 128@64^2 / 256@32^2, same box -- twice the LDS-DMA pieces per MFMA
    // cost more than the overlap buys; the kernel template still takes WN = 1 for the step)
    if (tile_rows == 65) return launch_step_t<1, 2, 2, 0, 2, 4, 1, 2>(a, s);   // 64 px as two K groups of 4 waves (160 KB, internal code)
    // 256 px as 16 waves of 32 px x 128 columns (4 per SIMD, 114 VGPRs) instead of 8 of 64 x 128: bit-identical, -2...-4 % same box
    if (tile_rows == 256) return launch_step_t<1, 8, 2>(a, s);
    return tile_rows == 128 ? launch_step_t<1, 4, 3>(a, s) : launch_step_t<1, 2, 2>(a, s);
}

// the step's backward (EPI = 2): 64-pixel tiles of 4 waves (two workgroups per CU), the forward's 64-pixel instance with the backward epilogue
hipError_t launch_convlstm_step_bwd(const ConvLstmArgs &a, hipStream_t s) { return launch_step_t<1, 2, 2, 2>(a, s); }

// plain convolution (EPI = 1): Cout % 256 == 0 takes the 256-column tiles of the gate kernel (three pixel-tile sizes), Cout =
// 128 / 64 / 32 a 256-pixel tile of 4 waves with 4 / 2 / 1 column fragments per wave
int conv_tile_cols(int Cout) { return Cout % 256 == 0 ? 256 : (Cout == 128 || Cout == 64 || Cout == 32) ? Cout : 0; }

// like_b > 0: the automatic tile is chosen as for a batch of like_b images (a time-folded batch then runs the per-step launch's instance:
// the same summation order per image, bit for bit)
hipError_t launch_conv_nhwc(const ConvLstmArgs &a, int tile_rows, hipStream_t s, int64_t like_b)
{
    const int64_t m = (like_b > 0 ? like_b : (int64_t)a.B) * a.H * a.W;
    const int cus = device_cus();
    // halo tiles (conv_halo_kernel): the 16 x 16 patch with its halo staged once per 64-channel chunk.  One patch buffer + two
    // weight-group buffers must leave room for TWO workgroups per CU (<= 80 KB): 8 clips of 256^2, same box, 5x5: 64 -> 32
    // columns 0.117 -> 0.085 ms (3 taps per group), 128 -> 64 columns 0.079 -> 0.071 ms (1 tap); 256 -> 128 columns does not fit
    // twice and measured 0.126-0.137 against 0.090 ms on the 128-pixel tile; with one workgroup per CU (two patch buffers or
    // 5-tap groups) the same kernel is slower than the tiles above; an 8-row patch (30 KB, so that 128 columns fit twice) measured
    // 0.109 against 0.090 ms as well.  tile_rows 16 forces it (tests), 0 takes it where measured.
    const int halo_a = conv_halo_pieces(a.ks) * 1024;
    const int halo_tps = a.n_cols % 256 != 0 ? (80 * 1024 - halo_a) / (2 * a.n_cols * 128) : 0;
    const bool halo_ok = a.C % 64 == 0 && a.n_cols % 256 != 0 && a.stride == 1 && a.H % 16 == 0 && a.W % 16 == 0 && halo_tps >= 1;
    if (halo_ok && (tile_rows == 16 || (tile_rows == 0 && a.ks == 5 && a.n_cols <= 64))) {
        const int nf = a.n_cols / 32;
        const int tps = halo_tps < a.ks ? halo_tps : a.ks;
        const int lds = halo_a + 2 * tps * a.n_cols * 128;
        const void *fn = nf == 4 ? (const void *)&conv_halo_kernel<4> : nf == 2 ? (const void *)&conv_halo_kernel<2> : (const void *)&conv_halo_kernel<1>;
        static std::atomic<bool> raised[3][64];                              // once per instance and device
        const hipError_t e = ensure_dynamic_lds(fn, 160 * 1024, raised[nf == 4 ? 2 : nf - 1]);
        if (e != hipSuccess) return e;
        const unsigned tiles = (unsigned)(a.B * (a.H / 16) * (a.W / 16));
        if (nf == 4) hipLaunchKernelGGL(conv_halo_kernel<4>, dim3(tiles), dim3(256), lds, s, a, tps);
        else if (nf == 2) hipLaunchKernelGGL(conv_halo_kernel<2>, dim3(tiles), dim3(256), lds, s, a, tps);
        else hipLaunchKernelGGL(conv_halo_kernel<1>, dim3(tiles), dim3(256), lds, s, a, tps);
        return hipGetLastError();
    }
    if (a.C == 32) {                                                 // two taps per chunk (the UNet's first encoder: 32 -> 64, 5x5, stride 2)
        if (tile_rows == 0) tile_rows = (m / 256 >= cus) ? 256 : 128;
        if (a.n_cols == 64) return tile_rows == 256 ? launch_step_t<2, 4, 2, 1, 1, 2, 2>(a, s) : tile_rows == 128 ? launch_step_t<1, 4, 3, 1, 1, 2, 2>(a, s) : hipErrorInvalidValue;
        if (a.n_cols == 128) return tile_rows == 256 ? launch_step_t<2, 4, 2, 1, 1, 4, 2>(a, s) : tile_rows == 128 ? launch_step_t<1, 4, 3, 1, 1, 4, 2>(a, s) : hipErrorInvalidValue;
        return hipErrorInvalidValue;
    }
    if (a.n_cols % 256 != 0) {
        // one column tile of 4 / 2 / 1 B fragments per wave: 256 pixels (8 fragment rows of 4 waves x MF 2), or 128 pixels on
        // three stages when 256-pixel tiles leave CUs idle (8 clips at 64^2, same box: 5x5 256 -> 128 121 -> 88 us, 5x5
        // stride-2 64 -> 128 41 -> 30 us).  Measured and not kept for 32 columns: 512- and 256-pixel tiles of MF 4 (+26 / +41 %)
        if (tile_rows == 0) tile_rows = (m / 256 >= cus) ? 256 : 128;
        if (tile_rows == 256) {
            if (a.n_cols == 128) return launch_step_t<2, 4, 2, 1, 1, 4>(a, s);
            if (a.n_cols == 64) return launch_step_t<2, 4, 2, 1, 1, 2>(a, s);
            if (a.n_cols == 32) return launch_step_t<2, 4, 2, 1, 1, 1>(a, s);
        } else if (tile_rows == 128) {
            // 128 columns: two K groups of 4 waves on two stages each (128 KB) instead of 4 waves on three: same box, 8 clips at
            // 64^2, 5x5 256 -> 128 87.7 -> 72.4 us, stride-2 64 -> 128 29.4 -> 26.1 us
            if (a.n_cols == 128) return launch_step_t<1, 4, 2, 1, 1, 4, 1, 2>(a, s);
            if (a.n_cols == 64) return launch_step_t<1, 4, 3, 1, 1, 2>(a, s);
            if (a.n_cols == 32) return launch_step_t<1, 4, 3, 1, 1, 1>(a, s);
        }
        return hipErrorInvalidValue;
    }
    if (tile_rows == 0) {
        const int64_t ct = a.n_cols / kClBN;
        // 32-pixel tiles when even 64-pixel ones leave CUs idle (8 clips at 32^2, same box: residual-block convolution 36.7 ->
        // 30.0 us, 5x5 stride-2 128 -> 256 48.0 -> 39.1 us; a third stage on the 64-pixel tile measured no gain)
        // ... and better still 64 px x 128 columns, i.e. half a packed column tile per workgroup (4 waves of 32 x 64, three
        // stages): a third fewer LDS-DMA pieces per MFMA than 32 px x 256 columns (30.1 -> 27.4 us, 39.2 -> 36.0 us), and with the
        // workgroup as two K groups of 4 waves (KS = 2: 8 waves, 144 KB) 31.0 -> 24.3 us and 39.7 -> 30.2 us on the same box
        tile_rows = (m / 256 * ct >= cus) ? 256 : (m / 128 * ct >= cus) ? 128 : (m / 64 * ct < cus) ? 66 : 64;
    }
    if (tile_rows == 256) return launch_step_t<2, 4, 2, 1>(a, s);
    if (tile_rows == 32) return launch_step_t<1, 1, 3, 1, 4, 2>(a, s); // 4 waves of 32 px x 64 columns, three stages
    if (tile_rows == 66) {                                             // 64 px x HALF a packed column tile (internal code, see above)
        ConvLstmArgs b = a;
        b.pack_cols = kClBN;
        return launch_step_t<1, 2, 3, 1, 2, 2, 1, 2>(b, s);            // ... as two K groups of 4 waves (see the kernel's KS)
    }
    return tile_rows == 128 ? launch_step_t<1, 4, 3, 1>(a, s) : launch_step_t<1, 2, 2, 1>(a, s);
}

hipError_t launch_conv_pack(const float *w, uint16_t *wp, int Cin, int Cout, int ks, hipStream_t s)
{
    if (Cin == 32) {
        const int64_t n32 = (int64_t)Cout * ((ks * ks + 1) / 2) * kClBK;
        hipLaunchKernelGGL(conv_pack32_kernel, dim3((unsigned)((n32 + 255) / 256)), dim3(256), 0, s, w, wp, Cout, ks, conv_tile_cols(Cout));
        return hipGetLastError();
    }
    const int64_t n = (int64_t)Cout * Cin * ks * ks;
    hipLaunchKernelGGL(conv_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, wp, Cin, Cout, ks, conv_tile_cols(Cout));
    return hipGetLastError();
}

hipError_t launch_nchw_to_nhwc_bf16(const void *src, bool src_bf16, uint16_t *dst, int B, int C, int HW, int relu, hipStream_t s)
{
    const int64_t blocks = (int64_t)B * (C / 64) * (HW / 64);
    if (src_bf16)
        hipLaunchKernelGGL(nchw_to_nhwc_bf16_kernel<uint16_t>, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const uint16_t *>(src), dst, C, HW, relu);
    else
        hipLaunchKernelGGL(nchw_to_nhwc_bf16_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const float *>(src), dst, C, HW, relu);
    return hipGetLastError();
}

hipError_t launch_conv1x1_nhwc(const uint16_t *x, const uint16_t *skip, const float *w, const float *bias, void *out, int out_bf16, int64_t M,
                               int C, int Cout, hipStream_t s)
{
    const int64_t n = M * (C / 8);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    switch (Cout) {
    case 1: hipLaunchKernelGGL(conv1x1_nhwc_kernel<1>, grid, block, 0, s, x, skip, w, bias, out, out_bf16, M, C); break;
    case 2: hipLaunchKernelGGL(conv1x1_nhwc_kernel<2>, grid, block, 0, s, x, skip, w, bias, out, out_bf16, M, C); break;
    case 3: hipLaunchKernelGGL(conv1x1_nhwc_kernel<3>, grid, block, 0, s, x, skip, w, bias, out, out_bf16, M, C); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

namespace {
// one work-item per (image, segment of rs rows, column, 8 output channels).  8 clips, same box, us per launch (events) for
// rs = 1 / 2 / 4 / 8: 256 ch @32^2 17.1 / 18.0 / 17.9 / 23.8, 128 ch @64^2 23.0 / 20.7 / 20.0 / 22.6, 64 ch @128^2
// 38.1 / 30.0 / 25.6 / 30.8 -> 4 rows where that leaves >= 2048 waves, else 1 (tools/upsample_time.py).  The values do not depend
// on rs.  rs_forced > 0 takes that segment length instead.  Returns the work-items, or -1 when they do not fit the kernel's 32-bit index.
int64_t upsample2x_work(int B, int H, int W, int C, int rs_forced, int &rs)
{
    const int64_t cols = (int64_t)B * W * (C / 8);
    rs = rs_forced > 0 ? rs_forced : cols * ((H + 3) / 4) < 2048 * 64 ? 1 : 4;
    const int64_t n = cols * ((H + rs - 1) / rs);
    return n < (int64_t)1 << 31 ? n : -1;
}
}  // namespace

hipError_t launch_upsample2x_cat_nhwc(const uint16_t *x, int C1, const uint16_t *skip, int C2, uint16_t *out, int B, int H, int W, hipStream_t s)
{
    int rs;
    const int64_t n = upsample2x_work(B, H, W, C1 + C2, 0, rs);
    if (n < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(upsample2x_cat_nhwc_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, C1, skip, C2, out, B, H, W, rs);
    return hipGetLastError();
}

hipError_t launch_upsample2x_nhwc(const uint16_t *x, const uint16_t *skip, uint16_t *out, int B, int H, int W, int C, hipStream_t s)
{
    int rs, forced = 0;
#ifdef V2V_TUNING_KNOBS                                                           // tuning builds only (tools/upsample_time.py): never in the product launch path
    if (const char *e = getenv("V2V_UP_RS")) forced = atoi(e) > 0 ? atoi(e) : 4;
#endif
    const int64_t n = upsample2x_work(B, H, W, C, forced, rs);
    if (n < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(upsample2x_nhwc_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, skip, out, B, H, W, C, rs);
    return hipGetLastError();
}

}  // namespace v2v

using v2v::aligned;
using v2v::fail;
using v2v::hip_fail;
using v2v::launched;

extern "C" {

int v2v_convlstm_packed_bytes(int64_t C, uint64_t *bytes)
{
    if (!bytes) return fail(V2V_ERR_NULL, "v2v_convlstm_packed_bytes: bytes is NULL");
    if (C < 64 || C % 64 != 0) return fail(V2V_ERR_SHAPE, "ConvLSTM kernel needs C %% 64 == 0 (got %lld)", (long long)C);
    *bytes = (uint64_t)4 * C * 2 * C * 9 * 2;
    return V2V_OK;
}

int v2v_convlstm_pack_weights_hip(const float *gates_weight, int64_t C, void *packed, void *stream)
{
    if (!gates_weight || !packed) return fail(V2V_ERR_NULL, "v2v_convlstm_pack_weights_hip: gates_weight/packed is NULL");
    if (C < 64 || C % 64 != 0 || C > 4096) return fail(V2V_ERR_SHAPE, "ConvLSTM kernel needs C %% 64 == 0, C <= 4096 (got %lld)", (long long)C);
    if (!aligned(gates_weight, 4) || !aligned(packed, 16)) return fail(V2V_ERR_ALIGN, "gates_weight needs 4-byte, packed 16-byte alignment");
    const int64_t n = (int64_t)4 * C * 2 * C * 9;
    hipLaunchKernelGGL(v2v::convlstm_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), gates_weight,
                       static_cast<uint16_t *>(packed), (int)C);
    return launched("convlstm_pack_kernel launch");
}

int v2v_convlstm_step_hip(const void *x, const void *h_prev, const float *c_prev, const void *packed, const float *gates_bias,
                          int64_t B, int64_t H, int64_t W, int64_t C, void *h_state, float *c_state, void *h_nchw, int h_nchw_dtype, int tile_rows, void *stream)
{
    if (h_nchw && h_nchw_dtype != V2V_F32 && h_nchw_dtype != V2V_BF16) return fail(V2V_ERR_DTYPE, "h_nchw_dtype must be V2V_F32 or V2V_BF16");
    if (!x || !packed || !gates_bias || !h_state || !c_state) return fail(V2V_ERR_NULL, "v2v_convlstm_step_hip: x/packed/gates_bias/h_state/c_state is NULL");
    if (B < 1 || H < 1 || W < 1 || C < 64 || C % 64 != 0 || C > 4096) return fail(V2V_ERR_SHAPE, "need B,H,W >= 1 and C %% 64 == 0, C <= 4096");
    if (tile_rows != 0 && tile_rows != 64 && tile_rows != 128 && tile_rows != 256) return fail(V2V_ERR_PARAM, "tile_rows must be 0 (auto), 64, 128 or 256");
    if ((H * W) % 4 != 0 || B * H * W * C > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "ConvLSTM kernel needs (H*W) %% 4 == 0 and B*H*W*C < 2^31 (got %lldx%lldx%lldx%lld)",
                    (long long)B, (long long)H, (long long)W, (long long)C);
    if (h_state == h_prev || h_state == x) return fail(V2V_ERR_PARAM, "h_state must not alias h_prev or x (neighbouring tiles read them)");
    if (!aligned(x, 16) || !aligned(h_prev, 16) || !aligned(packed, 16) || !aligned(h_state, 2) || !aligned(c_prev, 4) || !aligned(c_state, 4) ||
        !aligned(gates_bias, 4) || !aligned(h_nchw, 16))
        return fail(V2V_ERR_ALIGN, "x/h_prev/packed/h_nchw need 16-byte alignment");
    v2v::ConvLstmArgs a{};
    a.x = static_cast<const uint16_t *>(x); a.h_prev = static_cast<const uint16_t *>(h_prev); a.c_prev = c_prev;
    a.wp = static_cast<const uint16_t *>(packed); a.bias = gates_bias;
    a.h_state = static_cast<uint16_t *>(h_state); a.c_state = c_state; a.h_nchw = h_nchw; a.h_nchw_bf16 = h_nchw_dtype == V2V_BF16;
    a.B = (int)B; a.H = (int)H; a.W = (int)W; a.C = (int)C;
    const hipError_t e = v2v::launch_convlstm_step(a, tile_rows, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? V2V_OK : hip_fail(e, "convlstm_step_kernel launch");
}

int64_t v2v_conv_packed_elems(int64_t Cin, int64_t Cout, int ks)
{
    if ((ks != 3 && ks != 5) || Cout < 1 || Cout > 4096 || v2v::conv_tile_cols((int)Cout) == 0) return -1;
    if (Cin == 32) return (Cout == 64 || Cout == 128) ? Cout * ((ks * ks + 1) / 2) * 64 : -1;      // two taps per 64-wide chunk
    if (Cin < 64 || Cin % 64 != 0 || Cin > 4096) return -1;
    return Cout * Cin * ks * ks;
}

int v2v_conv_pack_weights_hip(const float *weight, int64_t Cin, int64_t Cout, int ks, void *packed, void *stream)
{
    if (!weight || !packed) return fail(V2V_ERR_NULL, "v2v_conv_pack_weights_hip: weight/packed is NULL");
    if (v2v_conv_packed_elems(Cin, Cout, ks) < 0)
        return fail(V2V_ERR_SHAPE, "conv kernel needs Cin %% 64 == 0 (or Cin 32 with Cout 64 / 128), Cout in {32, 64, 128} or a multiple of 256, ks 3 or 5 (got %lld -> %lld, ks %d)",
                    (long long)Cin, (long long)Cout, ks);
    if (!aligned(weight, 4) || !aligned(packed, 16)) return fail(V2V_ERR_ALIGN, "weight needs 4-byte, packed 16-byte alignment");
    const hipError_t e = v2v::launch_conv_pack(weight, static_cast<uint16_t *>(packed), (int)Cin, (int)Cout, ks, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? V2V_OK : hip_fail(e, "conv_pack_kernel launch");
}

int v2v_conv_nhwc_hip(const void *x, const void *packed, const float *bias, const void *residual, int relu, int64_t B, int64_t Hin,
                      int64_t Win, int64_t Cin, int64_t Cout, int ks, int stride, void *out, int tile_rows, void *stream)
{
    if (!x || !packed || !bias || !out) return fail(V2V_ERR_NULL, "v2v_conv_nhwc_hip: x/packed/bias/out is NULL");
    if ((ks != 3 && ks != 5) || (stride != 1 && stride != 2)) return fail(V2V_ERR_PARAM, "ks must be 3 or 5, stride 1 or 2");
    if (B < 1 || Hin < 1 || Win < 1 || v2v_conv_packed_elems(Cin, Cout, ks) < 0)
        return fail(V2V_ERR_SHAPE, "need B,H,W >= 1, Cin %% 64 == 0 (or Cin 32 with Cout 64 / 128), Cout in {32, 64, 128} or a multiple of 256");
    const int64_t H = (Hin - 1) / stride + 1, W = (Win - 1) / stride + 1;          // output size for pad = ks / 2
    if (tile_rows != 0 && tile_rows != 128 && tile_rows != 256 && tile_rows != 16 && (Cout % 256 != 0 || (tile_rows != 32 && tile_rows != 64)))
        return fail(V2V_ERR_PARAM, "tile_rows must be 0 (auto), 128 or 256 (and 32 or 64 for Cout %% 256 == 0)");
    const bool halo_fits = Cin % 64 == 0 && Cout % 256 != 0 && stride == 1 && H % 16 == 0 && W % 16 == 0 && (ks == 3 || Cout <= 64);   // see launch_conv_nhwc
    const bool halo = halo_fits && (tile_rows == 16 || (tile_rows == 0 && ks == 5));
    if (tile_rows == 16 && !halo) return fail(V2V_ERR_PARAM, "tile_rows 16 (halo tiles) needs stride 1, H and W multiples of 16 and Cout 32 / 64 (128 for 3x3)");
    if ((H * W) % 4 != 0 || B * Hin * Win * Cin > 0x7FFFFFFFLL || B * H * W * Cout > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "conv kernel needs (Hout*Wout) %% 4 == 0 and tensors below 2^31 elements");
    if (out == x) return fail(V2V_ERR_PARAM, "out must not alias x (neighbouring tiles read it)");
    if (!aligned(x, 16) || !aligned(packed, 16) || !aligned(out, 2) || !aligned(residual, 2) || !aligned(bias, 4))
        return fail(V2V_ERR_ALIGN, "x/packed need 16-byte alignment");
    v2v::ConvLstmArgs a{};
    a.x = static_cast<const uint16_t *>(x); a.wp = static_cast<const uint16_t *>(packed); a.bias = bias;
    a.residual = static_cast<const uint16_t *>(residual); a.out_nhwc = static_cast<uint16_t *>(out);
    a.n_cols = (int)Cout; a.relu = relu ? 1 : 0; a.ks = ks; a.stride = stride; a.Hin = (int)Hin; a.Win = (int)Win;
    a.B = (int)B; a.H = (int)H; a.W = (int)W; a.C = (int)Cin;
    const hipError_t e = v2v::launch_conv_nhwc(a, tile_rows, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? V2V_OK : hip_fail(e, "conv (convlstm_step_kernel, EPI = 1) launch");
}

int64_t v2v_conv_head_packed_elems(int ks) { return (ks == 3 || ks == 5) ? (int64_t)((ks * ks + 7) / 8) * 32 * 64 : -1; }

int v2v_conv_head_pack_weights_hip(const float *weight, int64_t Cin, int ks, void *packed, void *stream)
{
    if (!weight || !packed) return fail(V2V_ERR_NULL, "v2v_conv_head_pack_weights_hip: weight/packed is NULL");
    if (Cin < 1 || Cin > 8 || (ks != 3 && ks != 5)) return fail(V2V_ERR_SHAPE, "need 1 <= Cin <= 8 and ks 3 or 5 (32 output channels)");
    if (!aligned(packed, 16)) return fail(V2V_ERR_ALIGN, "packed needs 16-byte alignment");
    const int n = ((ks * ks + 7) / 8) * 32 * 64;
    hipLaunchKernelGGL(v2v::conv_head_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), weight,
                       static_cast<uint16_t *>(packed), (int)Cin, ks);
    return launched("conv_head_pack_kernel launch");
}

int v2v_to_nhwc8_bf16_hip(const float *src, int64_t stride_b, int64_t stride_c, int64_t stride_h, int64_t stride_w, int64_t B, int64_t C,
                          int64_t H, int64_t W, void *dst, void *stream)
{
    return v2v_to_nhwc8_bf16_scaled_hip(src, stride_b, stride_c, stride_h, stride_w, B, C, H, W, nullptr, dst, stream);
}

int v2v_to_nhwc8_bf16_scaled_hip(const float *src, int64_t stride_b, int64_t stride_c, int64_t stride_h, int64_t stride_w, int64_t B, int64_t C,
                                 int64_t H, int64_t W, const float *scales, void *dst, void *stream)
{
    if (!src || !dst) return fail(V2V_ERR_NULL, "v2v_to_nhwc8_bf16_hip: src/dst is NULL");
    if (B < 1 || C < 1 || C > 8 || H < 1 || W < 1 || B * H * W > 0x7FFFFFFFLL) return fail(V2V_ERR_SHAPE, "need B,H,W >= 1, 1 <= C <= 8, B*H*W < 2^31");
    if (!aligned(dst, 16) || !aligned(src, 4) || (scales && !aligned(scales, 4))) return fail(V2V_ERR_ALIGN, "dst needs 16-byte alignment");
    const int64_t n = B * H * W;
    hipLaunchKernelGGL(v2v::to_nhwc8_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), src, stride_b, stride_c,
                       stride_h, stride_w, static_cast<uint16_t *>(dst), (int)B, (int)C, (int)H, (int)W, scales);
    return launched("to_nhwc8_bf16_kernel launch");
}

int v2v_conv_head_nhwc_hip(const void *x8, const void *packed, const float *bias, int relu, int64_t B, int64_t H, int64_t W, int ks, void *out, void *stream)
{
    if (!x8 || !packed || !bias || !out) return fail(V2V_ERR_NULL, "v2v_conv_head_nhwc_hip: x8/packed/bias/out is NULL");
    if (ks != 3 && ks != 5) return fail(V2V_ERR_PARAM, "ks must be 3 or 5");
    if (B < 1 || H < 16 || W < 16 || H % 16 != 0 || W % 16 != 0 || B * H * W * 32 > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "need B >= 1, H and W multiples of 16, output below 2^31 elements");
    if (!aligned(x8, 16) || !aligned(packed, 16) || !aligned(out, 2) || !aligned(bias, 4)) return fail(V2V_ERR_ALIGN, "x8/packed need 16-byte alignment");
    const int pw = 16 + 2 * (ks >> 1), lds = ((pw * pw * 16 + 16 + 127) & ~127) + ((ks * ks + 7) / 8) * 32 * 128;
    hipLaunchKernelGGL(v2v::conv_head_kernel, dim3((unsigned)(B * (H / 16) * (W / 16))), dim3(256), lds, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(x8), static_cast<const uint16_t *>(packed), bias, static_cast<uint16_t *>(out), (int)B, (int)H, (int)W, ks,
                       relu ? 1 : 0);
    return launched("conv_head_kernel launch");
}

int v2v_conv1x1_nhwc_hip(const void *x, const void *skip, const float *weight, const float *bias, int64_t M, int64_t C, int64_t Cout,
                         void *out, int out_dtype, void *stream)
{
    if (!x || !weight || !bias || !out) return fail(V2V_ERR_NULL, "v2v_conv1x1_nhwc_hip: x/weight/bias/out is NULL");
    if (out_dtype != V2V_F32 && out_dtype != V2V_BF16) return fail(V2V_ERR_DTYPE, "out_dtype must be V2V_F32 or V2V_BF16");
    if (M < 1 || C < 8 || C > 512 || (C & (C - 1)) != 0 || Cout < 1 || Cout > 3 || M * (C / 8) > 0x7FFFFFFFLL * 256)
        return fail(V2V_ERR_SHAPE, "need M >= 1, C a power of two in 8..512, Cout 1..3");
    if (!aligned(x, 16) || !aligned(skip, 16) || !aligned(out, out_dtype == V2V_F32 ? 4 : 2)) return fail(V2V_ERR_ALIGN, "x/skip need 16-byte alignment");
    const hipError_t e = v2v::launch_conv1x1_nhwc(static_cast<const uint16_t *>(x), static_cast<const uint16_t *>(skip), weight, bias, out,
                                                  out_dtype == V2V_BF16, M, (int)C, (int)Cout, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? V2V_OK : hip_fail(e, "conv1x1_nhwc_kernel launch");
}

int v2v_upsample2x_nhwc_hip(const void *x, const void *skip, int64_t B, int64_t H, int64_t W, int64_t C, void *out, void *stream)
{
    if (!x || !out) return fail(V2V_ERR_NULL, "v2v_upsample2x_nhwc_hip: x/out is NULL");
    if (B < 1 || H < 1 || W < 1 || C < 8 || C % 8 != 0 || B * H * W * C > (1LL << 36))
        return fail(V2V_ERR_SHAPE, "need B,H,W >= 1, C %% 8 == 0 and an input below 2^36 elements");
    if (!aligned(x, 16) || !aligned(out, 16) || !aligned(skip, 16)) return fail(V2V_ERR_ALIGN, "x/skip/out need 16-byte alignment");
    if (out == x || out == skip) return fail(V2V_ERR_PARAM, "out must not alias x or skip");
    const hipError_t e = v2v::launch_upsample2x_nhwc(static_cast<const uint16_t *>(x), static_cast<const uint16_t *>(skip), static_cast<uint16_t *>(out),
                                                     (int)B, (int)H, (int)W, (int)C, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? V2V_OK : hip_fail(e, "upsample2x_nhwc_bf16_kernel launch");
}

int v2v_conv3x3_pack_weights_hip(const float *weight, int64_t Cin, int64_t Cout, void *packed, void *stream)
{
    return v2v_conv_pack_weights_hip(weight, Cin, Cout, 3, packed, stream);
}

int v2v_conv3x3_nhwc_hip(const void *x, const void *packed, const float *bias, const void *residual, int relu, int64_t B, int64_t H,
                         int64_t W, int64_t Cin, int64_t Cout, void *out, int tile_rows, void *stream)
{
    return v2v_conv_nhwc_hip(x, packed, bias, residual, relu, B, H, W, Cin, Cout, 3, 1, out, tile_rows, stream);
}

int v2v_nchw_to_nhwc_bf16_hip(const void *src, int src_dtype, int64_t B, int64_t C, int64_t H, int64_t W, int relu, void *dst, void *stream)
{
    if (!src || !dst) return fail(V2V_ERR_NULL, "v2v_nchw_to_nhwc_bf16_hip: src/dst is NULL");
    if (src_dtype != V2V_F32 && src_dtype != V2V_BF16) return fail(V2V_ERR_DTYPE, "src_dtype must be V2V_F32 or V2V_BF16");
    if (B < 1 || H < 1 || W < 1 || C < 64 || C % 64 != 0 || (H * W) % 64 != 0 || B * (C / 64) * (H * W / 64) > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "need B,H,W >= 1, C %% 64 == 0, (H*W) %% 64 == 0");
    if (!aligned(src, src_dtype == V2V_F32 ? 4 : 2) || !aligned(dst, 2)) return fail(V2V_ERR_ALIGN, "buffers misaligned");
    const hipError_t e = v2v::launch_nchw_to_nhwc_bf16(src, src_dtype == V2V_BF16, static_cast<uint16_t *>(dst), (int)B, (int)C, (int)(H * W),
                                                       relu ? 1 : 0, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? V2V_OK : hip_fail(e, "nchw_to_nhwc_bf16_kernel launch");
}

// the data gradient of a convolution runs on the forward convolution's instances (weights packed by v2v_conv_dgrad_pack_weights_hip,
// v2v_train_tu.hip), so its entry point lives with them
int v2v_conv_dgrad_nhwc_hip(const void *dy, const void *packed, const void *residual, int64_t B, int64_t Hin, int64_t Win, int64_t Cin, int64_t Cout,
                            int ks, int stride, void *workspace, void *dx, void *stream)
{
    if (!dy || !packed || !workspace || !dx) return fail(V2V_ERR_NULL, "v2v_conv_dgrad_nhwc_hip: dy/packed/workspace/dx is NULL");
    if ((ks != 3 && ks != 5) || (stride != 1 && stride != 2)) return fail(V2V_ERR_PARAM, "ks must be 3 or 5, stride 1 or 2");
    if (B < 1 || Hin < 1 || Win < 1 || v2v_conv_dgrad_packed_elems(Cin, Cout, ks) < 0 || Hin % stride != 0 || Win % stride != 0 || (Hin * Win) % 4 != 0
        || B * Hin * Win * (Cin > Cout ? Cin : Cout) > 0x7FFFFFFFLL || Cout % 8 != 0)
        return fail(V2V_ERR_SHAPE, "need the transposed convolution Cout -> Cin to be a shape the convolution kernel takes, Hin, Win multiples "
                                   "of the stride, (Hin*Win) %% 4 == 0, tensors below 2^31 elements");
    if (dx == dy) return fail(V2V_ERR_PARAM, "dx must not alias dy");
    if (!aligned(dy, 16) || !aligned(packed, 16) || !aligned(workspace, 256) || !aligned(dx, 2) || !aligned(residual, 2))
        return fail(V2V_ERR_ALIGN, "dy/packed need 16-byte, workspace 256-byte alignment");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    float *zero_bias = static_cast<float *>(workspace);
    hipError_t e = hipMemsetAsync(zero_bias, 0, Cin * 4, s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(zero bias)");
    const uint16_t *src = static_cast<const uint16_t *>(dy);
    if (stride == 2) {
        uint16_t *grid = reinterpret_cast<uint16_t *>(static_cast<unsigned char *>(workspace) + (Cin * 4 + 255) / 256 * 256);
        e = v2v::launch_relu_mask_stuff(src, nullptr, grid, (int)B, (int)(Hin / 2), (int)(Win / 2), (int)Cout, 2, s);
        if (e != hipSuccess) return hip_fail(e, "relu_mask_stuff_kernel launch");
        src = grid;
    }
    v2v::ConvLstmArgs a{};
    a.x = src; a.wp = static_cast<const uint16_t *>(packed); a.bias = zero_bias;
    a.residual = static_cast<const uint16_t *>(residual); a.out_nhwc = static_cast<uint16_t *>(dx);
    a.n_cols = (int)Cin; a.relu = 0; a.ks = ks; a.stride = 1; a.Hin = (int)Hin; a.Win = (int)Win;
    a.B = (int)B; a.H = (int)Hin; a.W = (int)Win; a.C = (int)Cout;
    e = v2v::launch_conv_nhwc(a, 0, s);
    return e == hipSuccess ? V2V_OK : hip_fail(e, "dgrad (convlstm_step_kernel, EPI = 1) launch");
}

// ---- the plain UNet (EVFlowNet): stem, concat-skip upsampling, the time-folded convolution ----------------------------------------------
int64_t v2v_conv_stem_packed_elems(void) { return 2 * 64 * 64; }

int v2v_conv_stem_pack_weights_hip(const float *weight, int64_t Cin, void *packed, void *stream)
{
    if (!weight || !packed) return fail(V2V_ERR_NULL, "v2v_conv_stem_pack_weights_hip: weight/packed is NULL");
    if (Cin < 1 || Cin > 8) return fail(V2V_ERR_SHAPE, "need 1 <= Cin <= 8 (64 output channels, 3x3)");
    if (!aligned(weight, 4) || !aligned(packed, 16)) return fail(V2V_ERR_ALIGN, "weight needs 4-byte, packed 16-byte alignment");
    hipLaunchKernelGGL(v2v::conv_stem_pack_kernel, dim3(2 * 64 * 64 / 256), dim3(256), 0, static_cast<hipStream_t>(stream), weight, static_cast<uint16_t *>(packed),
                       (int)Cin);
    return launched("conv_stem_pack_kernel launch");
}

int v2v_conv_stem_nhwc_hip(const void *x8, const void *packed, const float *bias, int relu, int64_t B, int64_t H, int64_t W, void *out, void *stream)
{
    if (!x8 || !packed || !bias || !out) return fail(V2V_ERR_NULL, "v2v_conv_stem_nhwc_hip: x8/packed/bias/out is NULL");
    if (B < 1 || H < 16 || W < 16 || H % 16 != 0 || W % 16 != 0 || B * H * W * 16 > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "need B >= 1, H and W multiples of 16, output below 2^31 elements");
    if (!aligned(x8, 16) || !aligned(packed, 16) || !aligned(out, 2) || !aligned(bias, 4)) return fail(V2V_ERR_ALIGN, "x8/packed need 16-byte alignment");
    if (out == x8) return fail(V2V_ERR_PARAM, "out must not alias x8");
    hipLaunchKernelGGL(v2v::conv_stem_kernel, dim3((unsigned)(B * (H / (2 * v2v::kStemT)) * (W / (2 * v2v::kStemT)))), dim3(256), v2v::kStemLdsBytes,
                       static_cast<hipStream_t>(stream), static_cast<const uint16_t *>(x8), static_cast<const uint16_t *>(packed), bias,
                       static_cast<uint16_t *>(out), (int)B, (int)H, (int)W, relu ? 1 : 0);
    return launched("conv_stem_kernel launch");
}

int v2v_upsample2x_cat_nhwc_hip(const void *x, int64_t C1, const void *skip, int64_t C2, int64_t B, int64_t H, int64_t W, void *out, void *stream)
{
    if (!x || !out || (C2 > 0 && !skip)) return fail(V2V_ERR_NULL, "v2v_upsample2x_cat_nhwc_hip: x/out (or skip with C2 > 0) is NULL");
    if (B < 1 || H < 1 || W < 1 || C1 < 8 || C1 % 8 != 0 || C2 < 0 || C2 % 8 != 0 || B * 4 * H * W * (C1 + C2) > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "need B,H,W >= 1, C1 %% 8 == 0, C2 %% 8 == 0 and an output below 2^31 elements");
    if (skip && C2 == 0) return fail(V2V_ERR_PARAM, "skip given with C2 == 0");
    if (!aligned(x, 16) || !aligned(out, 16) || !aligned(skip, 16)) return fail(V2V_ERR_ALIGN, "x/skip/out need 16-byte alignment");
    if (out == x || out == skip) return fail(V2V_ERR_PARAM, "out must not alias x or skip");
    const hipError_t e = v2v::launch_upsample2x_cat_nhwc(static_cast<const uint16_t *>(x), (int)C1, static_cast<const uint16_t *>(skip), (int)C2,
                                                         static_cast<uint16_t *>(out), (int)B, (int)H, (int)W, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? V2V_OK : hip_fail(e, "upsample2x_cat_nhwc_bf16_kernel launch");
}

int v2v_conv_nhwc_like_hip(const void *x, const void *packed, const float *bias, const void *residual, int relu, int64_t B, int64_t Hin, int64_t Win,
                           int64_t Cin, int64_t Cout, int ks, int stride, void *out, int64_t B_like, void *stream)
{
    if (!x || !packed || !bias || !out) return fail(V2V_ERR_NULL, "v2v_conv_nhwc_like_hip: x/packed/bias/out is NULL");
    if ((ks != 3 && ks != 5) || (stride != 1 && stride != 2) || B_like < 0) return fail(V2V_ERR_PARAM, "ks must be 3 or 5, stride 1 or 2, B_like >= 0");
    if (B < 1 || Hin < 1 || Win < 1 || v2v_conv_packed_elems(Cin, Cout, ks) < 0)
        return fail(V2V_ERR_SHAPE, "need B,H,W >= 1, Cin %% 64 == 0 (or Cin 32 with Cout 64 / 128), Cout in {32, 64, 128} or a multiple of 256");
    const int64_t H = (Hin - 1) / stride + 1, W = (Win - 1) / stride + 1;
    if ((H * W) % 4 != 0 || B * Hin * Win * Cin > 0x7FFFFFFFLL || B * H * W * Cout > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "conv kernel needs (Hout*Wout) %% 4 == 0 and tensors below 2^31 elements");
    if (out == x) return fail(V2V_ERR_PARAM, "out must not alias x (neighbouring tiles read it)");
    if (!aligned(x, 16) || !aligned(packed, 16) || !aligned(out, 2) || !aligned(residual, 2) || !aligned(bias, 4))
        return fail(V2V_ERR_ALIGN, "x/packed need 16-byte alignment");
    v2v::ConvLstmArgs a{};
    a.x = static_cast<const uint16_t *>(x); a.wp = static_cast<const uint16_t *>(packed); a.bias = bias;
    a.residual = static_cast<const uint16_t *>(residual); a.out_nhwc = static_cast<uint16_t *>(out);
    a.n_cols = (int)Cout; a.relu = relu ? 1 : 0; a.ks = ks; a.stride = stride; a.Hin = (int)Hin; a.Win = (int)Win;
    a.B = (int)B; a.H = (int)H; a.W = (int)W; a.C = (int)Cin;
    const hipError_t e = v2v::launch_conv_nhwc(a, 0, static_cast<hipStream_t>(stream), B_like);
    return e == hipSuccess ? V2V_OK : hip_fail(e, "conv (convlstm_step_kernel, EPI = 1) launch");
}

}  // extern "C"
