"""The NAM cell's three launches under CO-SCHEDULING with matrix-core work on another stream, built like
tests/test_convgru_concurrency.py: a ConvLSTM step / a rocBLAS bf16 GEMM runs on a second stream while the cell runs, and every output --
the three bf16 operands, their fp32 masters, alpha and o_pre -- must be the stand-alone one bit for bit (the library is built without
packed float32 instructions; the epilogues are scalar float32)."""
import pytest
import torch

from test_convgru_concurrency import _disturbers

pytestmark = pytest.mark.gpu


def _victim(c, hw):
    from nam_stock import nam_case
    from v2v_amd import nhwc_ops as N
    x, m, h, cp, ws = nam_case(8, c, hw, hw, seed=9 + c)
    nhwc = lambda t, dt=torch.bfloat16: t.permute(0, 2, 3, 1).contiguous().cuda().to(dt)        # noqa: E731
    xn, mn, hn, cn = nhwc(x), nhwc(m), nhwc(h), nhwc(cp, torch.float32)
    packed = N.pack_nam_weights(*(ws[k].cuda() for k in ("conv_x", "conv_h", "conv_m", "conv_o", "conv_last", "lag")))
    return lambda: tuple(N.nam_step(xn, mn, hn, cn, packed, return_workspaces=True).values())


@pytest.mark.parametrize("c,hw", [(64, 48), (128, 24), (256, 12)])
def test_nam_step_does_not_depend_on_what_shares_the_cu(c, hw):
    run = _victim(c, hw)
    side = torch.cuda.Stream()
    solo = run()
    torch.cuda.synchronize()
    assert all(float(o.float().abs().max()) > 0 for o in solo)
    for name, disturb in _disturbers().items():
        for rep in range(4):
            with torch.cuda.stream(side):
                for _ in range(24):
                    disturb()
            outs = [run() for _ in range(4)]
            torch.cuda.synchronize()
            for o in outs:
                for k, (a, b) in enumerate(zip(o, solo)):
                    assert torch.equal(a, b), f"NAM output {k} differs from its stand-alone result while {name} runs on another stream ({int((a != b).sum())} elements)"
