"""The image-loss kernels (v2v_amd/csrc/v2v_loss.hpp) under CO-SCHEDULING with matrix-core work on another stream, built like
tests/test_firenet_concurrency.py: a ConvLSTM step / a rocBLAS bf16 GEMM runs on a second stream while the sequence losses run forward and
backward, and the loss tables and the gradient must be the stand-alone ones bit for bit (the library is built without packed float32
instructions; the scatter accumulates in integers)."""
import pytest
import torch

import loss_inputs as LI
from test_convgru_concurrency import _disturbers

pytestmark = pytest.mark.gpu


def test_sequence_losses_do_not_depend_on_what_shares_the_cu():
    from v2v_amd import loss_ops
    inp = {k: torch.from_numpy(v).cuda() for k, v in LI.seq_inputs().items()}

    def run():
        pred = inp["pred"].clone().requires_grad_(True)
        out = loss_ops.sequence_losses(pred, inp["frame"], inp["flow"], 1.0, 1.0, 1.0, LI.SEQ_L0)
        sum(v.sum() for v in out.values()).backward()
        return [v.detach() for v in out.values()] + [pred.grad]
    side = torch.cuda.Stream()
    solo = run()
    torch.cuda.synchronize()
    assert all(float(o.abs().max()) > 0 for o in solo)
    for name, disturb in _disturbers().items():
        for rep in range(6):
            with torch.cuda.stream(side):
                for _ in range(24):
                    disturb()
            outs = [run() for _ in range(4)]
            torch.cuda.synchronize()
            for o in outs:
                for k, (a, b) in enumerate(zip(o, solo)):
                    assert torch.equal(a, b), f"loss output {k} differs from its stand-alone result while {name} runs on another stream ({int((a != b).sum())} elements)"
