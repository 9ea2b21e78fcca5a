"""The ConvGRU step's two launches (gates, candidate) under CO-SCHEDULING with matrix-core work on another stream, built like
tests/test_hyper_concurrency.py: a ConvLSTM step / a rocBLAS bf16 GEMM runs on a second stream while the step runs, and every output --
bf16 state, fp32 state, update gate, h * reset -- must be the stand-alone one (the library is built without packed float32 instructions,
DESIGN 4.9; the epilogues blend in scalar float32)."""
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


def _victim(c, hw):
    from v2v_amd import convlstm as CL
    g = torch.Generator().manual_seed(9 + c)
    x = torch.randn((12, hw, hw, c), generator=g).bfloat16().cuda()
    h32 = torch.tanh(torch.randn((12, hw, hw, c), generator=g)).cuda()
    hb = h32.bfloat16()
    packed = CL.pack_gru_weights(*((torch.randn((c, 2 * c, 3, 3), generator=g) * 0.03).cuda() for _ in range(3)))
    b_gates, b_out = (torch.randn(2 * c, generator=g) * 0.3).cuda(), (torch.randn(c, generator=g) * 0.3).cuda()
    return lambda: CL.convgru_step(x, hb, h32, packed, b_gates, b_out)


@pytest.mark.parametrize("c,hw", [(64, 64), (128, 32), (256, 16)])
def test_convgru_step_does_not_depend_on_what_shares_the_cu(c, hw):
    run = _victim(c, hw)
    side = torch.cuda.Stream()
    solo = run()
    torch.cuda.synchronize()
    assert all(float(o.float().abs().max()) > 0 for o in solo)
    for name, disturb in _disturbers().items():
        for rep in range(6):
            with torch.cuda.stream(side):
                for _ in range(24):
                    disturb()
            outs = [run() for _ in range(4)]
            torch.cuda.synchronize()
            for o in outs:
                for k, (a, b) in enumerate(zip(o, solo)):
                    assert torch.equal(a, b), f"ConvGRU output {k} differs from its stand-alone result while {name} runs on another stream ({int((a != b).sum())} elements)"
