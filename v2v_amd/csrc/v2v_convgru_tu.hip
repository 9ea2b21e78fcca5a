// v2v_convgru_tu.hip -- translation unit of the ConvGRU step: the EPI = 3 (gates) and EPI = 4 (candidate) instances of convlstm_step_kernel
// and their launchers.  Kernel main loop in v2v_convlstm.hpp, epilogues / packing / layouts in v2v_convgru.hpp.
#include "v2v_convgru.hpp"
#include "v2v_args.hpp"

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

hipError_t launch_convgru_pack(const float *w_u, const float *w_r, const float *w_o, uint16_t *wp_gates, uint16_t *wp_cand, int C, hipStream_t s)
{
    const int64_t n = (int64_t)3 * C * 2 * C * 9;
    hipLaunchKernelGGL(convgru_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w_u, w_r, w_o, wp_gates, wp_cand, C);
    return hipGetLastError();
}

}  // namespace v2v
