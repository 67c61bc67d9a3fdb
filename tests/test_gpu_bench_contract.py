"""bench.py's driver contract, exercised end to end on one GPU: ONE JSON line with the contract's keys, and the
multi-GPU code path (process group over RCCL, per-step gather to the merge rank, max-over-ranks timing) with world
size 1 (PREMVOS_BENCH_FORCE_DIST=1) -- the 8-GPU launch itself is the driver's."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra_env, *args):
    env = dict(os.environ, **extra_env)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, env=env,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_line_through_the_distributed_path():
    d = _run({"PREMVOS_BENCH_FORCE_DIST": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29533", "RANK": "0",
              "WORLD_SIZE": "1", "LOCAL_RANK": "0"}, "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2",
             "--scaling", "weak", "--full", "--no-cpu-baseline", "--file-to-file", "0", "--supplementary", "none")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak" and d["dtype"] == "f32"
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert abs(d["value"] - 2 * 1000.0 / d["ms_per_step"]) < 1e-2 * d["value"]          # frames / time, whole job
    assert d["value"] > 10.0                                                               # an MI355X does > 10 frames/s
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 157.3
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and 20 < r["achieved"] < r["mfma_ceiling_measured"] <= 160
    assert "workload" in d["config"] and "model" not in d["config"]
    assert "ONE" in d["config"]["parallelism"] and "gather" in d["config"]["parallelism"]
    assert r["traffic"] is None or "profiles/" in r["traffic_source"]
    # the line carries its own box factors: HBM copy rate, one canonical layer, clock / power over the timed region
    assert 2000 < r["hbm_ceiling_measured"] < 8000 and r["canonical_layer"]["us"] > 0 and "728 -> 728" in r["canonical_layer"]["what"]
    assert "error" in d["box"] or (d["box"]["samples"] >= 1 and 500 < d["box"]["sclk_mhz_mean_of_xcds"]["mean"] < 3000)
    sr = r["mfma_ceiling_sustained_random_data"]              # the pure MFMA loop on changing random operands, sustained: <= the burst on constants
    assert 100 < sr["tflops"] <= r["mfma_ceiling_measured"] * 1.01 and sr["seconds"] >= 1.0
    # the roofline leg's own clock sample and the peak / family fraction at that clock (`frac` itself stays priced at the nominal peak)
    assert "error" in r["leg_box"] or (r["peak_at_granted_clock"] <= 157.3 * 1.02 and
                                       abs(r["igemm_family_frac_at_granted_clock"] * r["peak_at_granted_clock"] - r["igemm_family_frac"] * 157.3) < 0.5)
    # ... and per-rank scaling diagnostics whenever a process group exists
    pr = d["per_rank"]
    assert len(pr["ms_per_step"]) == 1 and pr["rank_skew_ms_per_step"] == 0.0 and pr["exchange_wait_ms_per_step"][0] >= 0.0
    assert pr["cold_start_s"][0] > 0 and d["cold_start_s"] == pr["cold_start_s"][0]
    # round 6: the whole launch priced against the same peak (every kernel of a frame, the timed region's own wall time), and a cold
    # start that no longer counts the synthesis of weights / frames on the host
    gf = d["config"]["gflop_per_frame"]
    assert abs(r["whole_step_frac"] - 2 * gf * 1e9 / (r["whole_step_ms_per_launch"] * 1e-3) / 1e12 / 157.3) < 2e-3
    assert 0.05 < r["whole_step_frac"] < r["frac"] + 0.05 and abs(r["non_conv_ms_per_launch"] - (r["whole_step_ms_per_launch"] - r["conv_ms_per_step"])) < 1e-2
    cs = d["cold_start"]
    assert abs(cs["build_pipeline_s"] + cs["first_launch_s"] - d["cold_start_s"]) < 0.03 and cs["synthetic_inputs_s"] > 0
    assert d["cold_start_s"] < 30 and d["box"].get("device_matched_by", "pci").startswith(("pci", "position"))


def test_a_plain_bench_run_carries_the_headline_only():
    """Without --full the line is what its headline figure needs: no roofline replay, file-to-file or merge-ingest leg,
    supplementary modes or CPU baseline run after the timed region, even when no option switches them off."""
    d = _run({}, "--gpus", "1", "--steps", "1", "--warmup", "1", "--batch", "2", "--frames", "2")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "data", "config"):
        assert k in d, k
    assert d["steps"] == 1 and d["warmup"] == 1 and d["dtype"] == "f32" and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert abs(d["value"] - 2 * 1000.0 / d["ms_per_step"]) < 1e-2 * d["value"]
    for k in ("roofline", "file_to_file", "merge_ingest", "supplementary", "cpu_baseline"):
        assert k not in d, k


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` outside torch.distributed spawns the ranks itself; with the gloo backend two ranks may share
    the one GPU of the test box (RCCL, the product backend, needs a device per rank)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update({"PREMVOS_BENCH_BACKEND": "gloo", "HSA_ENABLE_IPC_MODE_LEGACY": "0", "PREMVOS_AUTOTUNE": "0"})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch",
                        "2", "--scaling", "weak", "--no-cpu-baseline", "--no-roofline", "--file-to-file", "0"], capture_output=True, text=True, env=env, timeout=1500)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["frames_per_launch_per_gpu"] == 2 and d["scaling"] == "weak"
    assert abs(d["value"] - 2 * 2 * 1000.0 / d["ms_per_step"]) < 1e-2 * d["value"]      # whole-job frames / max-over-ranks time


def test_bench_strong_scaling_shards_one_video_over_two_ranks():
    """The default mode: ONE synthetic video shared out by premvos_amd.parallel.plan_shards -- 7 frame pairs in chunks of 2 over
    two ranks = ranges [0,4) and [4,7): rank 0 reads frame 4 as the second image of its last pair, rank 1's last chunk is ragged
    (one frame, padded to the launch batch, counted once).  value = frames of the video / max-over-ranks time per pass."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update({"PREMVOS_BENCH_BACKEND": "gloo", "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch",
                        "2", "--frames", "7", "--no-cpu-baseline", "--no-roofline", "--file-to-file", "0"], capture_output=True, text=True, env=env,
                       timeout=1500)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["frames_per_step"] == 7
    assert abs(d["value"] - 7 * 1000.0 / d["ms_per_step"]) < 1e-2 * d["value"]
    assert d["conv_configurations"]["signatures_explored_by_time"] == 0                   # nothing was chosen by wall clock


def test_bench_refuses_more_ranks_than_gpus():
    import torch
    n = torch.cuda.device_count() + 1
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PREMVOS_BENCH_BACKEND")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "GPU" in (r.stderr + r.stdout)


def test_bench_strong_scaling_three_ranks_with_a_ragged_video():
    """Three ranks over gloo on the one test GPU: with the test process, bench.py's launcher and the
    torch.distributed.run agent, six processes hold the GPU, the most a shared box allows.  3 frame pairs in chunks of 2 = 2 chunks
    over 3 ranks -- one rank owns no chunk and only takes part in the gathers, the last chunk is ragged.  The line counts the 3 frames
    once.  (The world-8 plans and gathers: tests/test_cpu_parallel.py.)"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update({"PREMVOS_BENCH_BACKEND": "gloo", "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--steps", "2", "--warmup", "1", "--batch",
                        "2", "--frames", "3", "--no-cpu-baseline", "--no-roofline", "--file-to-file", "0"], capture_output=True, text=True,
                       env=env, timeout=2400)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 3 and d["scaling"] == "strong" and d["config"]["frames_per_step"] == 3
    assert abs(d["value"] - 3 * 1000.0 / d["ms_per_step"]) < 1e-2 * d["value"]
    # per-rank scaling diagnostics: one entry per rank, the chunk-less rank launches nothing
    pr = d["per_rank"]
    assert all(len(pr[k]) == 3 for k in ("ms_per_step", "launches_per_step", "exchange_wait_ms_per_step", "cold_start_s"))
    assert sorted(pr["launches_per_step"]) == [0, 1, 1] and sum(pr["launches_per_step"]) == 2
    assert pr["rank_skew_ms_per_step"] == round(max(pr["ms_per_step"]) - min(pr["ms_per_step"]), 3) and 0 <= pr["slowest_rank"] < 3
    assert max(pr["ms_per_step"]) <= d["ms_per_step"] * 1.001 and all(w >= 0 for w in pr["exchange_wait_ms_per_step"])
    assert d["conv_configurations"]["signatures_explored_by_time"] == 0


def test_bench_dumps_what_its_last_timed_step_computed(tmp_path):
    """--dump-outputs DIR: the result dicts of every chunk of the last timed step, the video's frames in order (the ragged chunk's
    padding left out), as float .npy files of at most 64 MB -- the same numbers FramePipeline computes for those frames in this
    process; an output over its cap is the seeded sample of its flat elements."""
    import zlib
    import numpy as np
    import torch
    from premvos_amd import synth
    from premvos_amd.pipeline import FramePipeline
    B, T, P, H, W = 2, 3, 20, 480, 854
    out = tmp_path / "dump"
    d = _run({}, "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", str(B), "--frames", str(T), "--no-cpu-baseline",
             "--no-roofline", "--file-to-file", "0", "--supplementary", "none", "--dump-outputs", str(out))
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    names = ("flow", "masks", "conf", "general_boxes", "general_probs", "general_count", "specific_boxes", "specific_probs",
             "specific_count")
    assert sorted(d["dumped_outputs"]["arrays"]) == sorted(names) and sorted(os.listdir(out)) == sorted(n + ".npy" for n in names)
    dumped = {n: np.load(out / (n + ".npy")) for n in names}
    assert sum(a.nbytes for a in dumped.values()) <= 64 << 20
    assert all(a.dtype == (np.float64 if n.endswith("_count") else np.float32) for n, a in dumped.items())

    pipe = FramePipeline(synth.pwc_state_dict(0), synth.proposal_weights(0), synth.proposal_weights(1), synth.refinement_weights(0),
                         batch=B, device="cuda", boxes_per_frame=P, precision="fp32", flow_precision="fp32")
    clip, boxes = synth.clip_frames(0, T + 1, H, W).cuda(), synth.clip_boxes(0, T, P, H, W).cuda()
    want = {n: [] for n in names}
    for c0 in range(0, T, B):
        n = min(B, T - c0)
        fr = [c0 + min(i, n - 1) for i in range(B)]            # a ragged chunk repeats its last frame, as bench.py pads it
        r = pipe.step(clip[fr].contiguous(), clip[[f + 1 for f in fr]].contiguous(), boxes[fr].contiguous())
        for k in names:
            want[k].append(r[k][:n].cpu())
    for k in names:
        full = torch.cat(want[k]).numpy()
        if dumped[k].shape == full.shape:
            ref = full
        else:                                                   # flow (2.5 M elements) is kept whole, masks (24.6 M) as 8 Mi
            assert k == "masks" and dumped[k].shape == (8 << 20,)
            idx = np.sort(np.random.default_rng(zlib.crc32(k.encode())).choice(full.size, 8 << 20, replace=False, shuffle=False))
            ref = full.reshape(-1)[idx]
        assert np.array_equal(dumped[k], ref.astype(dumped[k].dtype)), k
