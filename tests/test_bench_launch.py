"""bench.py --gpus N: the launcher starts N ranks itself when torchrun did not (the driver's `python bench.py --gpus N`
form), checks WORLD_SIZE against --gpus under torchrun, and reports the process group's world size."""
import json
import os
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import pytest

REPO = Path(__file__).resolve().parent.parent


def _bench():
    sys.path.insert(0, str(REPO))
    import bench
    return bench


def _args(**kw):
    a = dict(gpus=None, workload="score", no_cpu_baseline=True, cpu_seconds=1.0, full=False)
    a.update(kw)
    return SimpleNamespace(**a)


def test_single_rank_runs_in_process():
    b = _bench()
    assert b.launch_command(_args(gpus=None), {}, []) is None
    assert b.launch_command(_args(gpus=1), {}, ["--gpus", "1"]) is None


def test_n_ranks_are_launched_through_torchrun():
    b = _bench()
    argv = ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    cmd = b.launch_command(_args(gpus=4), {}, argv, port=29123)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index("--master-port") + 1] == "29123"
    assert Path(cmd[len(cmd) - len(argv) - 1]) == REPO / "bench.py"
    assert cmd[-len(argv):] == argv  # the children get the same flags (and see WORLD_SIZE, so they do not relaunch)


def test_under_torchrun_world_size_must_match():
    b = _bench()
    assert b.launch_command(_args(gpus=2), {"WORLD_SIZE": "2"}, []) is None
    assert b.launch_command(_args(gpus=None), {"WORLD_SIZE": "8"}, []) is None
    with pytest.raises(SystemExit, match="WORLD_SIZE=2"):
        b.launch_command(_args(gpus=4), {"WORLD_SIZE": "2"}, [])


def test_parent_measures_cpu_baseline_and_hands_it_to_the_ranks(monkeypatch):
    """With --full the parent runs the CPU baseline (no GPU in this process) and passes it to the children in the
    environment; its exit status is the children's."""
    b = _bench()
    monkeypatch.setattr(b, "cpu_baseline", lambda s: {"value": 1.5, "unit": "videos/s", "cores": 3})
    probe = [sys.executable, "-c", "import json, os, sys; d = json.loads(os.environ['VGE_BENCH_CPU_BASELINE']); "
                                   "sys.exit(0 if d['cores'] == 3 else 5)"]
    assert b.launch_ranks(_args(gpus=2, no_cpu_baseline=False, full=True), probe) == 0
    assert b.launch_ranks(_args(gpus=2, no_cpu_baseline=False, full=True),
                          [sys.executable, "-c", "import sys; sys.exit(7)"]) == 7


def test_plain_run_measures_no_cpu_baseline(monkeypatch):
    """Without --full the parent of a multi-rank `score` run starts its ranks at once: no CPU baseline is measured or
    handed on; the other workloads keep theirs."""
    b = _bench()

    def never(*a, **k):
        raise AssertionError("a plain run measured the CPU baseline")
    monkeypatch.setattr(b, "cpu_baseline", never)
    monkeypatch.delenv("VGE_BENCH_CPU_BASELINE", raising=False)
    probe = [sys.executable, "-c", "import os, sys; sys.exit(5 if 'VGE_BENCH_CPU_BASELINE' in os.environ else 0)"]
    assert b.launch_ranks(_args(gpus=2, no_cpu_baseline=False), probe) == 0
    assert b.plain_run(_args()) and not b.plain_run(_args(full=True)) and not b.plain_run(_args(workload="cfg5"))
    with pytest.raises(AssertionError, match="plain run"):
        b.launch_ranks(_args(gpus=2, no_cpu_baseline=False, workload="cfg5"), probe)


def test_full_and_dump_outputs_are_options_off_by_default():
    b = _bench()
    a = b.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = b.parse_args(["--full", "--dump-outputs", "somewhere"])
    assert a.full and a.dump_outputs == "somewhere"


def test_dump_outputs_keeps_small_arrays_whole_and_samples_large_ones_by_a_fixed_seed(tmp_path):
    """--dump-outputs: float32 / float64 arrays as <name>.npy, at most the limit in all; an array over its share is a
    row sample that is the same in every run (rows in ascending order), so two builds can be compared row for row."""
    import numpy as np
    b = _bench()
    rng = np.random.default_rng(5)
    arrays = {"ac": rng.normal(size=37).astype(np.float32), "tc": rng.normal(size=37),
              "seq_embed": rng.normal(size=(1000, 64)).astype(np.float32)}
    info = b.dump_outputs(tmp_path / "a", arrays, limit_bytes=3 * 64 * 4 * 100)   # 100 rows of seq_embed per share
    b.dump_outputs(tmp_path / "b", arrays, limit_bytes=3 * 64 * 4 * 100)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert np.array_equal(got["ac"], arrays["ac"]) and got["ac"].dtype == np.float32
    assert np.array_equal(got["tc"], arrays["tc"]) and got["tc"].dtype == np.float64
    assert got["seq_embed"].shape == (100, 64) and info["seq_embed"]["sampled_rows"] == 100
    assert info["ac"]["sampled_rows"] is None
    assert sum(g.nbytes for g in got.values()) <= 3 * 64 * 4 * 100
    assert np.array_equal(got["seq_embed"], np.load(tmp_path / "b" / "seq_embed.npy"))
    rows = [int(np.flatnonzero((arrays["seq_embed"] == r).all(axis=1))[0]) for r in got["seq_embed"]]
    assert rows == sorted(set(rows))
    # a second rank of a multi-rank run writes beside rank 0's files, not over them
    b.dump_outputs(tmp_path / "a", {"ac": arrays["ac"]}, rank=1, world=2)
    assert (tmp_path / "a" / "ac.rank1.npy").exists()


def test_gather_rank_times_two_gloo_ranks(tmp_path):
    """The per-rank (seconds, videos) all-gather on a world-size-2 gloo group: every rank sees both, in rank order."""
    code = (
        "import os, sys, json, torch, torch.distributed as dist\n"
        f"sys.path.insert(0, {str(REPO)!r})\n"
        "import bench\n"
        "dist.init_process_group('gloo')\n"
        "r = dist.get_rank()\n"
        "got = bench.gather_rank_times(1.0 + r, 256 + r, dist.get_world_size(), 'cpu')\n"
        f"open(os.path.join({str(tmp_path)!r}, f'r{{r}}.json'), 'w').write(json.dumps(got))\n"
        "dist.destroy_process_group()\n")
    script = tmp_path / "g.py"
    script.write_text(code)
    port = _bench()._free_port()
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                    "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)], check=True, timeout=300)
    for r in range(2):
        assert json.loads((tmp_path / f"r{r}.json").read_text()) == [[1.0, 256], [2.0, 257]]


@pytest.mark.gpu
def test_bench_gpus_2_launches_two_ranks():
    """`python bench.py --gpus 2 --full` (no torchrun) on the one-GPU box: two ranks (gloo, both on cuda:0) each score their
    256 clips; the line reports the process group's world size, both ranks, and value = all videos / the slowest rank."""
    env = dict(os.environ, VGE_BENCH_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--full", "--no-cpu-baseline", "--no-throughput-mode"], env=env, capture_output=True, text=True,
                       timeout=600, cwd=str(REPO))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["ranks_seen"] == 2 and out["backend"] == "gloo"
    assert out["config"]["parallelism"] == "video-sharded x2"
    per = out["per_rank_videos_per_s"]
    assert len(per) == 2
    slowest = min(per)  # every rank scores 256 clips per step, so the slowest rank has the lowest rate
    assert out["value"] == pytest.approx(2 * slowest, rel=1e-9)
    assert out["precision"]["max_abs_ac"] < 1e-4 and out["precision"]["max_abs_tc"] < 1e-4


def test_f16_conv_kernel_choice_follows_the_library(monkeypatch):
    """bench.py names the f16 mode's conv kernel (roofline `kernel`, the PMC entry it accepts) by the rule vge_api.cpp
    applies: the staggered x3s kernel in single fp16 unless VGE_F16_X3S=0 or the stems are split (VGE_F16_MIX bit 0)."""
    bench = _bench()
    monkeypatch.delenv("VGE_F16_X3S", raising=False)
    monkeypatch.delenv("VGE_F16_MIX", raising=False)
    assert bench.f16_conv_is_x3s()
    monkeypatch.setenv("VGE_F16_MIX", "0")
    assert bench.f16_conv_is_x3s()
    monkeypatch.setenv("VGE_F16_MIX", "3")
    assert not bench.f16_conv_is_x3s()
    monkeypatch.setenv("VGE_F16_MIX", "2")
    monkeypatch.setenv("VGE_F16_X3S", "0")
    assert not bench.f16_conv_is_x3s()


def test_pmc_traffic_refuses_a_pass_of_the_other_f16_kernel(monkeypatch):
    """The committed f16 PMC pass counts for the bench line only while it was taken on the kernel the line runs."""
    bench = _bench()
    pj = json.loads((REPO / "profiles" / "pmc_conv_encoder.json").read_text())
    monkeypatch.delenv("VGE_F16_X3S", raising=False)
    monkeypatch.delenv("VGE_F16_MIX", raising=False)
    got = bench.pmc_traffic("f16", 256)
    if pj["f16"].get("source_sha") == bench._kernel_sources_sha():
        assert (got is not None) == (pj["f16"]["kernel"] == "conv_encoder_x3s_kernel")
    monkeypatch.setenv("VGE_F16_X3S", "0")
    if pj["f16"]["kernel"] == "conv_encoder_x3s_kernel":
        assert bench.pmc_traffic("f16", 256) is None


def test_nested_e2e_record_failure_is_recorded_not_raised():
    """The config-3 record of the --full line runs as a child process (bench.py --workload e2e, 1 step after 1
    warm-up); when it cannot run (here: no GPU) the record says why and the config-2 line still prints."""
    if __import__("torch").cuda.is_available():
        pytest.skip("CPU-only check of the failure path")
    b = _bench()
    rec = b.run_e2e_child(SimpleNamespace(e2e_clips=2, e2e_timeout=300.0))
    assert "error" in rec and rec["error"].startswith("exit status"), rec
    assert "--workload e2e --clips 2 --steps 1 --warmup 1" in rec["cmd"]
    json.dumps(rec)


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_steps_outputs(tmp_path):
    """A plain `score` run in this process: --steps sets the timed steps, the line carries the headline keys and none
    of the --full records, and --dump-outputs holds what the last timed step computed: AC / TC per video and the
    window embeddings they were scored from (AC of a one-window video = || normalize(seq_embed) - centroid || <= 2).
    A second run with the same arguments scores identical inputs: identical files."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    b = _bench()
    dev = torch.device("cuda", 0)
    outs = []
    for d in ("a", "b"):
        args = b.apply_defaults(b.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1",
                                              "--dump-outputs", str(tmp_path / d)]))
        line = b.run_score(args, 1, 0, dev)
        outs.append({n: np.load(tmp_path / d / f"{n}.npy") for n in ("ac", "tc", "seq_embed", "tc_windows")})
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "f32x3" and line["unit"] == "videos/s"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(256 * 1e3 / line["ms_per_step"], rel=1e-9)
    for k in ("precision", "cpu_baseline", "throughput_mode", "e2e", "roofline", "stage_ms", "stage_roofline"):
        assert k not in line, k
    json.dumps(line)
    o = outs[0]
    assert o["ac"].shape == (256,) and o["ac"].dtype == np.float32
    assert o["tc"].shape == (256,) and o["tc"].dtype == np.float64
    assert o["seq_embed"].shape == (256, 256) and o["seq_embed"].dtype == np.float32
    assert o["tc_windows"].shape == (256,) and o["tc_windows"].dtype == np.float32
    assert all(np.isfinite(v).all() for v in o.values())
    assert (o["ac"] >= 0).all() and (o["ac"] <= 2.0 + 1e-6).all() and np.abs(o["seq_embed"]).max() > 0
    # one window per clip: a video's TC is its window's term (float32, widened)
    assert np.array_equal(o["tc"], o["tc_windows"].astype(np.float64))
    for n in o:
        assert np.array_equal(o[n], outs[1][n]), n
