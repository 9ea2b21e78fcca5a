"""Size-independent properties at BASELINE config-2 scale (no oracle needed) + the bench.py output contract."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_potential_conservation_full_size(luts):
    """Noise-free ESIM: every pixel's potential stays in (-C-, C+) after each reset, so
    L(last) - L(first) - sum_k (on_k*C+ - off_k*C-) = p_final - p_init  lies in (-(C+ + C-), C+ + C-).
    Checked on 32 clips of the full 32x256x256 shape for symmetric and asymmetric thresholds, both input dtypes."""
    from v2v_amd import esim as E
    b, n, h, w = 32, 32, 256, 256
    lut = torch.from_numpy(luts["lut64"]).cuda()
    for dtype in (torch.uint8, torch.float32):
        frames = E.synth_clips(b, n, h, w, dtype=dtype, seed=77)
        for cp, cn in ((0.2, 0.2), (0.15, 0.4)):
            raw = E.esim_voxel_batch(frames, [cp, cn, 0, 0, 0], bin_mode="sum", num_bins=n - 1, seed=3, out_dtype=torch.float64)[:, 0]
            on = raw.clamp(min=0).sum(dim=1)
            off = (-raw).clamp(min=0).sum(dim=1)
            dl = lut[frames[:, -1].long()] - lut[frames[:, 0].long()]
            resid = dl - (on * cp - off * cn)
            assert float(resid.abs().max()) < cp + cn + 1e-9
            # and the residual really is "final minus initial potential": initial is uniform in [-C-, C+)
            assert float(resid.max()) > 0.5 * (cp + cn) * 0.5 and float(resid.min()) < -0.25 * (cp + cn)


def test_linearity_of_binning_modes():
    """SUM with fpb=f equals the sum of f consecutive fpb=1 planes; bilinear bins are a fixed linear map of the raw
    per-pair counts (weights sum to 1 per pair)."""
    from v2v_amd import esim as E
    frames = E.synth_clips(8, 41, 128, 128, dtype=torch.uint8, seed=5)
    p = [0.2, 0.3, 0.05, 1e-3, 0.8]
    raw = E.esim_voxel_batch(frames, p, bin_mode="sum", num_bins=40, frames_per_bin=1, seed=9)          # [8,1,40,H,W]
    s5 = E.esim_voxel_batch(frames, p, bin_mode="sum", num_bins=5, frames_per_bin=2, seed=9)            # [8,4,5,H,W]
    assert torch.equal(s5, raw.reshape(8, 4, 5, 2, 128, 128).sum(dim=3))
    bil = E.esim_voxel_batch(frames, p, bin_mode="bilinear", num_bins=5, seed=9, out_dtype=torch.float64)
    k = torch.arange(40, dtype=torch.float64, device="cuda")
    t_norm = k / 39 * 4
    wts = torch.stack([(1 - (t_norm - bb).abs()).clamp(min=0) for bb in range(5)])                      # [5,40]
    want = torch.einsum("bk,nkhw->nbhw", wts, raw[:, 0].double())
    torch.testing.assert_close(bil, want, rtol=1e-12, atol=1e-12)


def test_bench_contract_json():
    """bench.py --full prints ONE JSON line with the contract's keys (small batch so it runs in seconds)."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "8",
                          "--full", "--cpu-budget", "1"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and "sample" in c
    assert d["parity_check"] == "ok"
    assert abs(d["value"] - 8 * 3 / (d["ms_per_step"] * 3e-3)) / d["value"] < 1e-6
    assert len(lines[0]) <= 4096 and res.stdout.strip().splitlines()[-1] == lines[0]


def test_bench_default_command_prints_a_small_last_line_and_a_sidecar(tmp_path):
    """The driver's command with --full (`python bench.py --gpus 1 --steps 20 --warmup 5 --full`: full batch, every default secondary
    workload, the loader bench, the CPU baseline).  Round 4's line had grown to 21.9 KB and the driver could not parse it: the contract
    line is the LAST non-empty stdout line, alone, at most 4 KB, and everything else sits in the sidecar file it names."""
    import time
    side = tmp_path / "bench_extra.json"
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--extra-out", str(side)],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert res.returncode == 0, res.stderr[-3000:]
    out_lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(out_lines) == 1, [l[:200] for l in out_lines]
    assert len(out_lines[-1].encode()) <= 4096
    d = json.loads(out_lines[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                "config", "roofline", "cpu_baseline", "parity_check", "dist_backend", "ms_per_step_per_rank"):
        assert key in d, key
    assert d["config"]["workload"] == "cfg2_esim_f32_256x32x256x256_bilinear5" and d["config"]["clips_per_gpu"] == 256 and d["steps"] == 20
    assert d["parity_check"] == "ok" and d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["cores"] == 1
    # north_star: "the reference CPU path timed on the same box's host cores in the same run (core count stated)" -- the NumPy port in a pool
    # over every core this process may USE (affinity mask cut by the cgroup quota, not os.cpu_count())
    ca = d["cpu_baseline_all_cores"]
    usable = len(os.sched_getaffinity(0))
    assert ca["kind"] == "port" and 1 <= ca["cores"] <= usable and ca["value"] > 0 and "worker processes" in ca["sample"]
    assert ca["cores"] == 1 or ca["value"] > d["cpu_baseline"]["value"]                                  # more cores, more grids per second
    for stream in (res.stderr,):                                                                       # the driver keeps stderr: nothing may abort
        assert "terminate called" not in stream and "Aborted" not in stream and "killed by signal" not in stream, stream[-2000:]
    r = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "algorithmic_bytes_per_launch", "kernel_ms_avg", "kernel_ms_p50"):
        assert key in r, key
    assert d["ms_per_step"] * d["steps"] / 1e3 <= wall                                                 # the driver's own consistency check
    extra = json.loads(side.read_text())
    assert "also_measured" in extra and "headline" in extra and len(extra["headline"]["kernel_ms_trace"]) == 20
    for name, rec in extra["also_measured"].items():
        assert "error" not in rec, (name, rec)
        if "parity_check" in rec:
            assert rec["parity_check"] == "ok", name
    lv = extra["also_measured"]["train_loader_b12_201x128x128"]["integration_levels_samples_per_s"]
    assert all(lv[k] and lv[k] > 0 for k in ("yaml_only_num_workers_0", "yaml_only_spawned_workers", "one_line_of_train_py_ring_loader",
                                             "reference_numpy_port_in_workers")), lv
    assert wall < 240, f"the default run took {wall:.0f} s"


def test_bench_plain_run_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """The plain command (no --full) sets up, warms up, times its K steps and prints the line: no parity guard, no CPU baseline, no
    settled-clock launches, no sidecar.  --dump-outputs writes what the last timed step computed: a seeded sample of the 256 clips'
    grids under 64 MB, equal bit for bit to the same launch made here on the same synthetic clips."""
    import bench
    from v2v_amd import esim
    dump, side = tmp_path / "dump", tmp_path / "bench_extra.json"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(dump),
                          "--extra-out", str(side)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    out_lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(out_lines) == 1, [l[:200] for l in out_lines]
    d = json.loads(out_lines[0])
    assert d["steps"] == 7 and d["warmup"] == 2 and d["config"]["clips_per_gpu"] == 256 and d["unit"] == "voxel grids/s" and d["dtype"] == "f64"
    assert abs(d["value"] - 256 * 7 / (d["ms_per_step"] * 7e-3)) / d["value"] < 1e-6 and d["higher_is_better"] is True
    assert d["parity_check"] is None and d["cpu_baseline"] is None and d["extra"] is None and "cpu_baseline_all_cores" not in d
    assert "kernel_ms_settled_p50" not in d["roofline"] and not side.exists()
    assert sorted(os.listdir(dump)) == ["voxels.npy"] and os.path.getsize(dump / "voxels.npy") <= 64e6
    got = np.load(dump / "voxels.npy")
    assert got.dtype == np.float32 and got.shape == (48, 5, 256, 256)
    idx = np.sort(np.random.default_rng(0).choice(256, 48, replace=False))
    wl = bench.WORKLOADS[bench.DEFAULT_WORKLOAD]
    frames = esim.synth_clips(256, wl["n"], wl["h"], wl["w"], dtype=torch.float32, seed=20240001, clip_id0=0, device="cuda")
    want = esim.esim_voxel_batch(frames, wl["params"], bin_mode="bilinear", num_bins=5, rng_mode="philox", seed=20240001, clip_id0=0)
    assert np.array_equal(got, want[torch.as_tensor(idx, device="cuda")].cpu().numpy())


def test_bench_two_ranks_under_torch_distributed_run():
    """The N > 1 path exactly as the driver launches it -- `python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2`
    -- on this 1-GPU box: both ranks share cuda:0 (--share-gpu) and rendezvous over gloo (RCCL refuses two ranks on one
    device).  Checks the JSON contract for N = 2: one line from rank 0, n_gpus 2, the backend that really ran, global clip ids
    per rank, an aggregate of BOTH ranks' grids."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--batch", "16",
           "--full", "--share-gpu", "--backend", "gloo"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-3000:])
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["dist_backend"] == "gloo" and d["scaling"] == "weak" and d["steps"] == 4
    assert d["config"]["clips_per_gpu"] == 16 and "2 GPU(s)" in d["config"]["sharding"]
    assert d["parity_check"] == "ok" and d["cpu_baseline"] is None and "also_measured" not in d        # rank-0-at-N=1 extras stay off
    assert len(lines[0].encode()) <= 4096 and res.stdout.strip().splitlines()[-1] == lines[0] and len(d["ms_per_step_per_rank"]) == 2
    assert abs(d["value"] - 2 * 16 * 4 / (d["ms_per_step"] * 4e-3)) / d["value"] < 1e-6                 # whole-job aggregate over both ranks
    single = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1", "--batch", "16",
                             "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    s1 = json.loads([l for l in single.stdout.splitlines() if l.startswith("{")][0])
    assert s1["dist_backend"] is None and 0.3 < d["value"] / s1["value"] < 2.5                          # two ranks on ONE device: ~1x, never 0


@pytest.mark.parametrize("workload,clips,grids_per_clip", [("train_loader_b12", 12, 40), ("cfg4_stream", 8, 1), ("cfg4_stream_staged", 8, 1)])
def test_bench_host_fed_stream_workloads_on_two_ranks(workload, clips, grids_per_clip):
    """`bench.py --gpus 2 --workload train_loader_b12 | cfg4_stream` as the driver would launch it (torch.distributed.run, two ranks sharing
    cuda:0 over gloo on this 1-GPU box): BASELINE configs 4 / 5 are host-fed streams, so these workloads put the host side -- worker
    processes, page-locked rings / staging buffers, the PCIe copy -- INSIDE the timed region (the headline shards a device-resident batch,
    which cannot fail to scale).  One line from rank 0: aggregate grids/s of both ranks, per-rank ms per step and PCIe GB/s."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "6", "--warmup", "2", "--workload", workload,
           "--full", "--share-gpu", "--backend", "gloo"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-3000:])
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0].encode()) <= 4096, res.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "voxel grids/sec" and d["n_gpus"] == 2 and d["dist_backend"] == "gloo" and d["config"]["workload"] == workload and d["config"]["host_fed"]
    assert abs(d["value"] - 2 * clips * grids_per_clip * 6 / (d["ms_per_step"] * 6e-3)) / d["value"] < 1e-6      # whole-job aggregate over both ranks
    st = d["stream"]
    assert abs(st["samples_per_s"] * grids_per_clip - d["value"]) / d["value"] < 1e-6
    assert len(st["pcie_GBps_per_rank"]) == 2 and all(0.05 < v < 70 for v in st["pcie_GBps_per_rank"]) and len(d["ms_per_step_per_rank"]) == 2
    assert st["h2d_bytes_per_step_per_rank"] > 1e6 and 0 < st["gpu_busy_fraction_rank0"] <= 1.5
    r = d["roofline"]
    assert r["bound"] == "hbm" and 0 < r["frac"] < 1 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12


def test_shapes_at_the_edges_vs_oracle(oracle_c, luts):
    """The reference's training shape (201 frames, 128x128, 40x5 bins), an odd-sized frame (scalar path, 101x203),
    and many tiny clips in one launch -- all bit-exact against the scalar C oracle."""
    from oracle import v2v_oracle as O
    from v2v_amd import esim as E
    p = [0.17, 0.23, 0.06, 1e-3, 0.9]
    train = O.synth_clip_s1(201, 128, 128, seed=1, dtype=np.uint8)[None]
    want, tot = oracle_c.esim_voxel(train, p, luts, seed=11, clip_id0=3, bin_mode=oracle_c.BIN_SUM, num_bins=5, frames_per_bin=1)
    c = torch.zeros((1, 2), dtype=torch.int64, device="cuda")
    got = E.esim_voxel_batch(torch.from_numpy(train).cuda(), p, num_bins=5, seed=11, clip_id0=3, counts=c)
    assert got.shape == (1, 40, 5, 128, 128) and np.array_equal(got.cpu().numpy(), want) and np.array_equal(c.cpu().numpy(), tot)
    odd = O.synth_clip_s1(12, 101, 203, seed=2, dtype=np.float32)[None]
    want, _ = oracle_c.esim_voxel(odd, p, luts, seed=5, bin_mode=oracle_c.BIN_BILINEAR, num_bins=4)
    got = E.esim_voxel_batch(torch.from_numpy(odd).cuda(), p, bin_mode="bilinear", num_bins=4, seed=5, out_dtype=torch.float64)
    assert np.array_equal(got.cpu().numpy(), want)
    tiny = np.stack([O.synth_clip_s1(6, 8, 8, seed=100 + i, dtype=np.uint8) for i in range(300)])
    params = np.tile(np.array(p), (300, 1))
    params[:, 0] += np.arange(300) * 1e-3
    want, tot = oracle_c.esim_voxel(tiny, params, luts, seed=9, clip_id0=1000, bin_mode=oracle_c.BIN_SUM, num_bins=5)
    c = torch.zeros((300, 2), dtype=torch.int64, device="cuda")
    got = E.esim_voxel_batch(torch.from_numpy(tiny).cuda(), params, num_bins=5, seed=9, clip_id0=1000, counts=c)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(c.cpu().numpy(), tot)


@pytest.mark.gpu
def test_entry_points_capture_into_a_hip_graph():
    """The C-ABI launches only enqueue work on the caller's stream (no allocation, no synchronisation): a front-end +
    simulator + v2e step captured in a hipGraph replays to the same bytes as eager launches."""
    import torch
    from v2v_amd import esim, frontend, v2e
    dev = torch.device("cuda")
    raw = torch.randint(0, 256, (2, 6, 96, 128, 3), dtype=torch.uint8, device=dev)
    table = torch.tensor([[3, 5, 80, 0], [10, 20, 70, 1]], dtype=torch.int32, device=dev)
    idx = torch.tensor([[0, 1, 2, 3, 4, 5]] * 2, dtype=torch.int32, device=dev)
    params = torch.tensor([0.2, 0.25, 0.05, 1e-3, 0.5], dtype=torch.float64, device=dev)
    vp = v2e.make_params(24, "pn_related", 0.5, 0.1, 0.0, 0.1, 30, 0.1, 0, 5.0, 0.1, 0.1)
    out_e = torch.empty((2, 1, 5, 64, 64), dtype=torch.float32, device=dev)
    out_v = torch.empty((2, 1, 5, 64, 64), dtype=torch.float32, device=dev)
    gray_keep = torch.empty((2, 6, 64, 64), dtype=torch.uint8, device=dev)

    def step():
        gray = frontend.prepare_clips_batch(raw, table, idx, 64, "gray", validate=False, max_crop_before=80)[1]
        gray_keep.copy_(gray)
        esim.esim_voxel_batch(gray, params, bin_mode="sum", num_bins=5, frames_per_bin=1, seed=9, out=out_e, validate=False)
        v2e.v2e_voxel_batch(gray, vp, bin_mode="sum", num_bins=5, frames_per_bin=1, seed=9, out=out_v)

    step()
    torch.cuda.synchronize()
    want = (gray_keep.clone(), out_e.clone(), out_v.clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for t in (gray_keep, out_e, out_v):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gray_keep, want[0]) and torch.equal(out_e, want[1]) and torch.equal(out_v, want[2])
    assert out_e.abs().sum() > 0 and out_v.abs().sum() > 0


def test_symmetric_hint_is_exact_and_loud(oracle_c, luts):
    """V2V_FLAG_SYMMETRIC (instances without the asymmetric loop, 4 waves per SIMD): bit-identical to the general kernel and to
    the C oracle for symmetric thresholds, both bin modes and input dtypes; auto-detected from host parameters; a clip that
    breaks the promise comes out as NaN (never as a wrong count), the other clips of the batch are unaffected."""
    from oracle import v2v_oracle as O
    from v2v_amd import esim
    b, n, h, w = 5, 11, 256, 256
    kw4 = dict(mapping="4px")                       # the hint has 4-pixel instances only (a batch this small would map 1 or 2 pixels)
    sym = [[0.2, 0.2, 0.1, 1e-3, 0.1], [0.35, 0.35, 0.05, 0.0, 0.0], [0.2, 0.2, 0.0, 2e-3, 0.3], [0.11, 0.11, 0.07, 1e-3, 0.2], [0.5, 0.5, 0.2, 0.0, 0.0]]
    for dt in (np.uint8, np.float32):
        video = np.stack([O.synth_clip_s1(n, h, w, seed=70 + i, dtype=dt) for i in range(b)])
        frames = torch.from_numpy(video).cuda()
        ptensor = torch.tensor(sym, dtype=torch.float64, device="cuda")
        for mode, kw in (("bilinear", dict(num_bins=5)), ("sum", dict(num_bins=5, frames_per_bin=2))):
            general = esim.esim_voxel_batch(frames, ptensor, bin_mode=mode, seed=3, symmetric=False, **kw, **kw4)     # device params: no auto-detection
            hinted = esim.esim_voxel_batch(frames, ptensor, bin_mode=mode, seed=3, symmetric=True, **kw, **kw4)
            auto = esim.esim_voxel_batch(frames, sym, bin_mode=mode, seed=3, **kw, **kw4)                              # host params: detected
            assert torch.equal(general, esim.esim_voxel_batch(frames, sym, bin_mode=mode, seed=3, **kw))                 # and the mapping the launcher picks
            assert torch.equal(general, hinted) and torch.equal(general, auto)
            bm = oracle_c.BIN_BILINEAR if mode == "bilinear" else oracle_c.BIN_SUM
            want, _ = oracle_c.esim_voxel(video, np.asarray(sym), luts, seed=3, bin_mode=bm, **kw)
            np.testing.assert_allclose(hinted.cpu().numpy(), want, rtol=1e-5, atol=1e-5)
            broken = [list(r) for r in sym]
            broken[2][1] = 0.25                                                                               # clip 2 is asymmetric now
            out = esim.esim_voxel_batch(frames, torch.tensor(broken, dtype=torch.float64, device="cuda"), bin_mode=mode, seed=3, symmetric=True, **kw, **kw4)
            assert bool(torch.isnan(out[2]).all()) and torch.equal(out[[0, 1, 3, 4]], general[[0, 1, 3, 4]])


@pytest.mark.gpu
@pytest.mark.parametrize("mapping", ["4px", "2px", "1px"])
def test_device_resident_parameters_outside_the_domain_poison_their_clip_only(mapping):
    """A [B,5] parameter table that lives on the device (the loaders' per-sample draws) cannot be checked by the host wrapper: a zero, negative,
    NaN or sub-1e-9 threshold, a negative or infinite noise parameter makes THAT clip NaN (+ the statistics' flag word) in the kernel's
    prologue -- never a wrong count -- and leaves the rest of the batch as it was.  The same values in a host list raise."""
    from v2v_amd import _lib, esim
    good = [0.2, 0.3, 0.05, 1e-3, 1.0]
    rows = [good, [0.0, 0.3, 0.05, 1e-3, 1.0], good, [0.2, -0.3, 0.05, 1e-3, 1.0], [float("nan"), 0.3, 0.05, 1e-3, 1.0], [1e-12, 0.3, 0.05, 1e-3, 1.0],
            [0.2, 0.3, -0.05, 1e-3, 1.0], [0.2, 0.3, 0.05, float("inf"), 1.0], [0.2, 0.3, 0.05, 1e-3, float("nan")], good]
    bad = [i for i, r in enumerate(rows) if r is not good]
    ok = [i for i, r in enumerate(rows) if r is good]
    frames = esim.synth_clips(len(rows), 11, 64, 64, dtype=torch.uint8, seed=12)
    clean = esim.esim_voxel_batch(frames, good, bin_mode="sum", num_bins=5, frames_per_bin=2, seed=3, mapping=mapping)
    for mode, kw in (("sum", dict(num_bins=5, frames_per_bin=2)), ("bilinear", dict(num_bins=5))):
        ref = esim.esim_voxel_batch(frames, good, bin_mode=mode, seed=3, mapping=mapping, **kw)
        stats = torch.zeros((len(rows), _lib.VOXEL_STATS_WORDS), dtype=torch.int32, device="cuda") if mode == "sum" else None
        out = esim.esim_voxel_batch(frames, torch.tensor(rows, dtype=torch.float64, device="cuda"), bin_mode=mode, seed=3, mapping=mapping, stats=stats, **kw)
        assert all(bool(torch.isnan(out[i]).all()) for i in bad) and torch.equal(out[ok], ref[ok])
        if stats is not None:
            flag = stats[:, 513].cpu().numpy()                                   # kStatBad: the word behind the 513 histogram bins
            assert all(flag[i] != 0 for i in bad) and all(flag[i] == 0 for i in ok)
    assert torch.equal(clean, ref if mode == "sum" else clean)
    for r in (rows[1], rows[5]):
        with pytest.raises(ValueError):
            esim.esim_voxel_batch(frames, r, bin_mode="sum", num_bins=5, frames_per_bin=2, seed=3)


@pytest.mark.parametrize("workload,batch", [("cfg4_pipeline_720p_to_256_41f_sum5", 2), ("cfg5_fused_convlstm_channels_last", 2)])
def test_bench_pipeline_workloads_run_with_two_ranks(workload, batch):
    """The configs BASELINE names for 8 GPUs (config 4: 720p -> front-end -> simulator; config 5: + the recurrent UNet) through the
    N > 1 path: two ranks on this box's one GPU (gloo), each with its own clips (global clip ids by rank), one JSON line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", str(batch),
                          "--workload", workload, "--full", "--share-gpu", "--backend", "gloo", "--hip-graph", "off"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-3000:])
    d = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["dist_world_size"] == 2 and d["config"]["workload"] == workload and d["config"]["clips_per_gpu"] == batch
    assert d["parity_check"] == "ok" and d["value"] > 0


def test_bench_gpus_n_without_a_launcher_starts_the_ranks_itself():
    """`python bench.py --gpus 2` with NO launcher and no WORLD_SIZE must not measure one GPU and call it two: bench.py starts the
    two ranks itself (torch.distributed.run child, before any GPU call in the parent) and relays rank 0's line.  Here both ranks
    share the box's one GPU over gloo; n_gpus, the world size the process group reports and one time per rank are in the line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "8",
                          "--full", "--share-gpu", "--backend", "gloo"], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-3000:])
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["dist_world_size"] == 2 and len(d["ms_per_step_per_rank"]) == 2 and d["dist_backend"] == "gloo"
    assert max(d["ms_per_step_per_rank"]) <= d["ms_per_step"] * 1.001 and d["parity_check"] == "ok"
