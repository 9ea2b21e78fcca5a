// v2v_convgru_tu.hip -- translation unit of the ConvGRU step: the EPI = 3 (gates) and EPI = 4 (candidate) instances of convlstm_step_kernel
// with their launchers and C entry points (include/v2v_hip.h).  Kernel main loop in v2v_convlstm.hpp, epilogues / packing / layouts in
// v2v_convgru.hpp.
#include "../../include/v2v_hip.h"
#include "v2v_convgru.hpp"
#include "v2v_args.hpp"
#include "v2v_status.hpp"

namespace v2v {

// Instance codes (v2v_convgru_step_hip's tile_gates / tile_cand; 0 = auto).  Pixels x columns per workgroup:
//   gates      1: 64 x 128    2: 128 x 128 (three stages)    3: 128 x 256 (three stages)    4: 256 x 256    5: 64 x 256 as two K groups
//   candidate  1: 128 x 64 (three stages)    2: 128 x 128 as two K groups    3: 128 x 256 (three stages)    4: 256 x 256    5: 64 x 128 as two K groups
// 256-column gate tiles need C % 128 == 0; candidate tiles of 128 / 256 columns C % 128 / C % 256 == 0.
bool convgru_tile_ok(int C, int tile_gates, int tile_cand)
{
    if (tile_gates < 0 || tile_gates > 5 || tile_cand < 0 || tile_cand > 5) return false;
    if (tile_gates >= 3 && C % 128 != 0) return false;
    const int cc = tile_cand == 1 ? 64 : (tile_cand == 2 || tile_cand == 5) ? 128 : tile_cand == 0 ? 64 : 256;
    return C % cc == 0;
}

// auto, by measurement (tools/convgru_time.py cell --tiles, profiles/convgru/tiles.jsonl; one MI355X, us per step for gates + candidate):
//   12 x 64 ch @64^2: 1+1 63, 2+1 75 | 12 x 128 ch @32^2: 1+5 66, 2+5 65, 5+5 68, 1+1 73, 1+2 81, 3+5 79, 4+5 97
//   12 x 256 ch @16^2: 1+5 102, 5+5 103, 1+1 116, 1+2 124, 1+3 156, 1+4 187, 3+5 130, 4+5 161
//   1 x 64 ch @96x120: 1+1 48, 2+1 46 | 1 x 128 ch @48x60: 1+5 58, 5+5 63, 1+1 69, 3+5 75 | 1 x 256 ch @24x30: 1+5 98, 5+5 101, 1+1 113, 3+5 129
// -> gates: the 64 x 128 tile (4 waves, 48 KB of LDS: three workgroups share a CU) wherever the 256-column tiles leave CUs idle; the K-split
// and the 128-pixel tile never beat it by more than 4 %.  Candidate: 64 x 128 as two K groups when C % 128 == 0, else 128 x 64.  The
// 256-column tiles are kept for launches that give every CU one (the rule of launch_convlstm_step, whose measurements it inherits).
hipError_t launch_convgru_gates(const ConvLstmArgs &a0, int tile, hipStream_t s)
{
    ConvLstmArgs a = a0;
    a.pack_cols = gru_gate_pack_cols(a.C);
    if (tile == 0) {
        const int cus = device_cus();
        const int64_t m = (int64_t)a.B * a.H * a.W;
        const bool wide = a.C % 128 == 0;
        const int64_t ctw = a.C / 128;
        tile = (wide && m / 256 * ctw >= cus) ? 4 : (wide && m / 128 * ctw >= cus) ? 3 : 1;
    }
    switch (tile) {
    case 1: return launch_step_t<1, 2, 2, 3, 2, 2>(a, s);
    case 2: return launch_step_t<1, 4, 3, 3, 2, 2>(a, s);
    case 3: return launch_step_t<1, 4, 3, 3, 2, 4>(a, s);
    case 4: return launch_step_t<1, 8, 2, 3, 2, 4>(a, s);
    case 5: return launch_step_t<1, 2, 2, 3, 2, 4, 1, 2>(a, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_convgru_candidate(const ConvLstmArgs &a0, int tile, hipStream_t s)
{
    ConvLstmArgs a = a0;
    a.pack_cols = gru_cand_pack_cols(a.C);
    if (tile == 0) {
        const int cus = device_cus();
        const int64_t m = (int64_t)a.B * a.H * a.W;
        if (a.C % 256 == 0 && m / 256 * (a.C / 256) >= cus) tile = 4;
        else if (a.C % 256 == 0 && m / 128 * (a.C / 256) >= cus) tile = 3;
        else if (a.C % 128 == 0) tile = 5;
        else tile = 1;
    }
    switch (tile) {
    case 1: return launch_step_t<1, 4, 3, 4, 1, 2>(a, s);
    case 2: return launch_step_t<1, 4, 2, 4, 1, 4, 1, 2>(a, s);
    case 3: return launch_step_t<1, 4, 3, 4, 2, 4>(a, s);
    case 4: return launch_step_t<1, 8, 2, 4, 2, 4>(a, s);
    case 5: return launch_step_t<1, 2, 3, 4, 2, 2, 1, 2>(a, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace v2v

using v2v::aligned;
using v2v::fail;
using v2v::hip_fail;
using v2v::launched;

extern "C" {

int v2v_convgru_packed_bytes(int64_t C, uint64_t *gates_bytes, uint64_t *cand_bytes)
{
    if (!gates_bytes || !cand_bytes) return fail(V2V_ERR_NULL, "v2v_convgru_packed_bytes: gates_bytes/cand_bytes is NULL");
    if (C < 64 || C % 64 != 0 || C > 4096) return fail(V2V_ERR_SHAPE, "ConvGRU kernel needs C %% 64 == 0, C <= 4096 (got %lld)", (long long)C);
    *gates_bytes = (uint64_t)2 * C * 2 * C * 9 * 2;
    *cand_bytes = (uint64_t)C * 2 * C * 9 * 2;
    return V2V_OK;
}

int v2v_convgru_pack_weights_hip(const float *update_weight, const float *reset_weight, const float *out_weight, int64_t C, void *packed_gates,
                                 void *packed_cand, void *stream)
{
    if (!update_weight || !reset_weight || !out_weight || !packed_gates || !packed_cand)
        return fail(V2V_ERR_NULL, "v2v_convgru_pack_weights_hip: a weight or packed pointer is NULL");
    if (C < 64 || C % 64 != 0 || C > 4096) return fail(V2V_ERR_SHAPE, "ConvGRU kernel needs C %% 64 == 0, C <= 4096 (got %lld)", (long long)C);
    if (!aligned(update_weight, 4) || !aligned(reset_weight, 4) || !aligned(out_weight, 4) || !aligned(packed_gates, 16) || !aligned(packed_cand, 16))
        return fail(V2V_ERR_ALIGN, "weights need 4-byte, packed streams 16-byte alignment");
    const int64_t n = (int64_t)3 * C * 2 * C * 9;
    hipLaunchKernelGGL(v2v::convgru_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), update_weight, reset_weight,
                       out_weight, static_cast<uint16_t *>(packed_gates), static_cast<uint16_t *>(packed_cand), (int)C);
    return launched("convgru_pack_kernel launch");
}

int v2v_convgru_step_hip(const void *x, const void *h_prev, const float *h_prev_f32, const void *packed_gates, const void *packed_cand,
                         const float *gates_bias, const float *out_bias, int64_t B, int64_t H, int64_t W, int64_t C, float *u_ws, void *hr_ws,
                         void *h_state, float *h_state_f32, void *h_nchw, int h_nchw_dtype, int tile_gates, int tile_cand, void *stream)
{
    if (h_nchw && h_nchw_dtype != V2V_F32 && h_nchw_dtype != V2V_BF16) return fail(V2V_ERR_DTYPE, "h_nchw_dtype must be V2V_F32 or V2V_BF16");
    if (!x || !packed_gates || !packed_cand || !gates_bias || !out_bias || !u_ws || !hr_ws || !h_state || !h_state_f32)
        return fail(V2V_ERR_NULL, "v2v_convgru_step_hip: x/packed_gates/packed_cand/gates_bias/out_bias/u_ws/hr_ws/h_state/h_state_f32 is NULL");
    if ((h_prev == nullptr) != (h_prev_f32 == nullptr)) return fail(V2V_ERR_NULL, "h_prev and h_prev_f32 come together (both NULL: the zero state)");
    if (B < 1 || H < 1 || W < 1 || C < 64 || C % 64 != 0 || C > 4096) return fail(V2V_ERR_SHAPE, "need B,H,W >= 1 and C %% 64 == 0, C <= 4096");
    if ((H * W) % 4 != 0 || B * H * W * C > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "ConvGRU kernel needs (H*W) %% 4 == 0 and B*H*W*C < 2^31 (got %lldx%lldx%lldx%lld)",
                    (long long)B, (long long)H, (long long)W, (long long)C);
    if (!v2v::convgru_tile_ok((int)C, tile_gates, tile_cand))
        return fail(V2V_ERR_PARAM, "tile_gates / tile_cand must be 0 (auto) or an instance code 1..5 whose columns divide C (got %d, %d for C = %lld)",
                    tile_gates, tile_cand, (long long)C);
    if (h_state == h_prev || h_state == x || h_state == hr_ws || hr_ws == h_prev || hr_ws == x || static_cast<void *>(u_ws) == static_cast<void *>(h_state_f32) ||
        u_ws == h_prev_f32)
        return fail(V2V_ERR_PARAM, "h_state / hr_ws must not alias x, h_prev or each other, u_ws not the fp32 states (neighbouring tiles read them)");
    if (!aligned(x, 16) || !aligned(h_prev, 16) || !aligned(hr_ws, 16) || !aligned(packed_gates, 16) || !aligned(packed_cand, 16) || !aligned(h_state, 2) ||
        !aligned(h_prev_f32, 4) || !aligned(h_state_f32, 4) || !aligned(u_ws, 4) || !aligned(gates_bias, 4) || !aligned(out_bias, 4) || !aligned(h_nchw, 16))
        return fail(V2V_ERR_ALIGN, "x/h_prev/hr_ws/packed_gates/packed_cand/h_nchw need 16-byte alignment");
    v2v::ConvLstmArgs g{};
    g.x = static_cast<const uint16_t *>(x); g.h_prev = static_cast<const uint16_t *>(h_prev); g.c_prev = h_prev_f32;
    g.wp = static_cast<const uint16_t *>(packed_gates); g.bias = gates_bias;
    g.h_state = static_cast<uint16_t *>(hr_ws); g.c_state = u_ws;
    g.B = (int)B; g.H = (int)H; g.W = (int)W; g.C = (int)C;
    hipError_t e = v2v::launch_convgru_gates(g, tile_gates, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "ConvGRU gates launch");
    v2v::ConvLstmArgs c{};
    c.x = g.x; c.h_prev = h_prev ? static_cast<const uint16_t *>(hr_ws) : nullptr; c.c_prev = h_prev_f32;
    c.wp = static_cast<const uint16_t *>(packed_cand); c.bias = out_bias; c.dh = u_ws;
    c.h_state = static_cast<uint16_t *>(h_state); c.c_state = h_state_f32; c.h_nchw = h_nchw; c.h_nchw_bf16 = h_nchw_dtype == V2V_BF16;
    c.B = (int)B; c.H = (int)H; c.W = (int)W; c.C = (int)C;
    e = v2v::launch_convgru_candidate(c, tile_cand, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? V2V_OK : hip_fail(e, "ConvGRU candidate launch");
}

}  // extern "C"
