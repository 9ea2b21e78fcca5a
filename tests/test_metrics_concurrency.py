"""The evaluation-metric kernels (v2v_amd/csrc/v2v_metrics.hpp) under CO-SCHEDULING with matrix-core work on another stream, built like
tests/test_loss_concurrency.py: a ConvLSTM step / a rocBLAS bf16 GEMM runs on a second stream while the image and the flow metrics of a
sequence are taken, and every output must be the stand-alone one bit for bit (no float atomics, slots added in a fixed order; the library is
built without packed float32 instructions)."""
import pytest
import torch

import metrics_reference as MR
from test_convgru_concurrency import _disturbers

pytestmark = pytest.mark.gpu


def test_metrics_do_not_depend_on_what_shares_the_cu():
    from v2v_amd import metrics
    pred, image = (torch.from_numpy(v).cuda() for v in MR.image_case("i180x240"))
    fp, fg, fe = (torch.from_numpy(v).cuda() for v in MR.flow_case("f180x240"))

    def run():
        out, smap = metrics.image_metrics(pred, image, ssim_map=True)
        counts, sums = metrics.flow_metrics(fp, fg, fe)
        return [out.view(torch.int64), smap.view(torch.int64), counts, sums.view(torch.int64)]
    side = torch.cuda.Stream()
    victim = torch.cuda.Stream()
    solo = run()
    torch.cuda.synchronize()
    assert all(int(o.abs().max()) > 0 for o in solo)
    for name, disturb in _disturbers().items():
        for rep in range(6):
            with torch.cuda.stream(side):
                for _ in range(24):
                    disturb()
            with torch.cuda.stream(victim):
                outs = [run() for _ in range(4)]
            torch.cuda.synchronize()
            for o in outs:
                for k, (a, b) in enumerate(zip(o, solo)):
                    assert torch.equal(a, b), f"metric output {k} differs from its stand-alone result while {name} runs on another stream ({int((a != b).sum())} elements)"
