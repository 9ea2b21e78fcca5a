"""The two new elementwise kernels of the plain UNet (the concat-skip upsampling and its adjoint) under CO-SCHEDULING with matrix-core work
on another stream, built like tests/test_hip_concurrency.py: a ConvLSTM step / a rocBLAS bf16 GEMM runs on a second stream while the
kernel runs, and every result must be the stand-alone one (the library is built without packed float32 instructions; these
kernels blend in float32 exactly like the upsampling kernel that showed the hazard)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _disturbers():
    from v2v_amd import convlstm as CL
    g = torch.Generator().manual_seed(5)
    c, hw = 64, 64
    xx = torch.randn((12, hw, hw, c), generator=g).bfloat16().cuda()
    hp = torch.randn((12, hw, hw, c), generator=g).bfloat16().cuda()
    cp = torch.randn((12, hw, hw, c), generator=g).cuda()
    packed = CL.pack_gate_weights((torch.randn((4 * c, 2 * c, 3, 3), generator=g) * 0.02).cuda())
    bias = torch.zeros(4 * c).cuda()
    a = torch.randn((2048, 2048), device="cuda").bfloat16()
    return {"convlstm_step": lambda: CL.convlstm_step(xx, hp, cp, packed, bias, nchw_dtype=None), "rocblas_bf16_mm": lambda: torch.mm(a, a)}


def _victims():
    from v2v_amd import nhwc_ops as ops
    g = torch.Generator().manual_seed(7)
    ux, usk = torch.randn((12, 64, 64, 64), generator=g).bfloat16().cuda(), torch.randn((12, 64, 64, 64), generator=g).bfloat16().cuda()
    du = torch.randn((12, 128, 128, 128), generator=g).bfloat16().cuda()
    return {"upsample2x_cat": lambda: ops.upsample2x_cat_nhwc(ux, usk),
            "upsample2x_cat_bwd": lambda: ops.upsample2x_cat_bwd_nhwc(du, 64, 64)}


@pytest.mark.parametrize("victim", ["upsample2x_cat", "upsample2x_cat_bwd"])
def test_new_elementwise_kernels_do_not_depend_on_what_shares_the_cu(victim):
    run = _victims()[victim]
    side = torch.cuda.Stream()
    solo = run()
    torch.cuda.synchronize()
    for name, disturb in _disturbers().items():
        for rep in range(6):
            with torch.cuda.stream(side):
                for _ in range(24):
                    disturb()
            outs = [run() for _ in range(4)]
            torch.cuda.synchronize()
            for o in outs:
                assert torch.equal(o, solo), f"{victim} differs from its stand-alone result while {name} runs on another stream ({int((o != solo).sum())} elements)"
