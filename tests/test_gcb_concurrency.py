"""The global context block's three launches and the valid-extent helper under CO-SCHEDULING with matrix-core work on another stream,
built like tests/test_convgru_concurrency.py: a ConvLSTM step / a rocBLAS bf16 GEMM runs on a second stream while the block runs, and the
output, the pooled context and the channel-add term must be the stand-alone ones bit for bit (float32 VALU arithmetic without packed
float32 instructions; a fixed-order reduction without atomics, so nothing depends on which workgroup finishes first)."""
import pytest
import torch

from test_convgru_concurrency import _disturbers

pytestmark = pytest.mark.gpu


def _victim(c, h, w, valid):
    from v2v_amd import nhwc_ops as N
    from gcb_stock import gcb_weights as _weights
    g = torch.Generator().manual_seed(17 + c)
    x = torch.randn((4, h, w, c), generator=g).bfloat16().cuda()
    packed = N.pack_gcb_weights(*(t.cuda() for t in _weights(c, g)))

    def run():
        out, ca = N.gcb_nhwc(x, packed, valid=valid, return_context=True)
        return out, ca, N.valid_extent_nhwc(out.clone(), valid, replicate=True)
    return run


@pytest.mark.parametrize("c,h,w,valid", [(32, 96, 128, (92, 120)), (64, 48, 64, (46, 60)), (128, 24, 32, (23, 30))])
def test_gcb_does_not_depend_on_what_shares_the_cu(c, h, w, valid):
    run = _victim(c, h, w, valid)
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
                    assert torch.equal(a, b), f"GCB output {k} differs from its stand-alone result while {name} runs on another stream ({int((a != b).sum())} elements)"
