"""HyperE2VID's new kernels (context staging, tanh, atoms, the dynamic convolution) under CO-SCHEDULING with matrix-core work on another
stream, built like tests/test_evflow_concurrency.py: a ConvLSTM step / a rocBLAS bf16 GEMM runs on a second stream while the kernel runs,
and every result must be the stand-alone one (the library is built without packed float32 instructions; the dynamic convolution
builds its features with float32 FMAs, the kind of arithmetic that showed the hazard)."""
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
    g = torch.Generator().manual_seed(9)
    ev, prev = torch.randn((12, 5, 128, 128), generator=g).cuda(), torch.randn((12, 1, 128, 128), generator=g).cuda()
    x = torch.randn((12, 32, 32, 256), generator=g).bfloat16().cuda()
    coeff = torch.randn((12, 32, 32, 128), generator=g).bfloat16().cuda()
    bases = torch.randn((12, 25), generator=g).cuda()
    atoms = (torch.randn((12, 32, 32, 25, 6), generator=g) * 0.3).cuda()
    packed = ops.pack_dynconv_weights((torch.randn((128, 1536, 1, 1), generator=g) * 0.03).cuda())
    bias = torch.randn(128, generator=g).cuda()
    cw, cb = torch.randn((32, 6, 3, 3), generator=g).cuda(), torch.randn(32, generator=g).cuda()
    return {"context": lambda: ops.context_conv_nhwc(ops.hyper_context_nhwc8(ev, prev), cw, cb), "atoms": lambda: ops.hyper_atoms(coeff, bases),
            "tanh": lambda: ops.tanh_bf16_(coeff.clone()), "dynconv": lambda: ops.dynconv_nhwc(x, atoms, packed, bias)}


@pytest.mark.parametrize("victim", ["context", "atoms", "tanh", "dynconv"])
def test_hyper_kernels_do_not_depend_on_what_shares_the_cu(victim):
    run = _victims()[victim]
    side = torch.cuda.Stream()
    solo = run()
    torch.cuda.synchronize()
    assert float(solo.float().abs().max()) > 0
    for name, disturb in _disturbers().items():
        for rep in range(6):
            with torch.cuda.stream(side):
                for _ in range(24):
                    disturb()
            outs = [run() for _ in range(4)]
            torch.cuda.synchronize()
            for o in outs:
                assert torch.equal(o, solo), f"{victim} differs from its stand-alone result while {name} runs on another stream ({int((o != solo).sum())} elements)"
