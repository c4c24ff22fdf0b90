"""The bench.py output contract (driver-facing): checks the latest committed bench line under profiles/ for every key
and type the task statement requires, and that bench.py's argument parser accepts the driver's command line."""
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _latest_bench_lines():
    """The newest round's committed bench lines: profiles/rNN_bench_<config>.json (one per BASELINE config)."""
    files = glob.glob(os.path.join(ROOT, "profiles", "r*_bench_*.json"))
    assert files, "no committed bench line under profiles/"
    rnd = max(int(re.match(r"r(\d+)_", os.path.basename(f)).group(1)) for f in files)
    return {os.path.basename(f).split("_bench_")[1][:-5]: json.load(open(f)) for f in files if os.path.basename(f).startswith(f"r{rnd:02d}_")}


def test_all_four_baseline_configs_have_a_committed_line():
    lines = _latest_bench_lines()
    assert set(lines) == {"embed", "frontend", "finetune", "stream"}
    assert lines["embed"]["config"]["workload"].startswith("configs[2]") and lines["frontend"]["config"]["workload"].startswith("configs[1]")
    assert lines["finetune"]["config"]["workload"].startswith("configs[3]") and lines["stream"]["config"]["workload"].startswith("configs[4]")
    assert lines["stream"]["unit"] == "windows/s" and lines["stream"]["latency_ms_batch1"] > 0
    assert lines["frontend"]["roofline"]["bound"] == "hbm" and lines["embed"]["roofline"]["bound"] == "mfma"
    builds = {d["config"]["build"] for d in lines.values()}
    assert len(builds) == 1                                            # one build, one box, one run of tools/gpu/evidence.sh


import pytest


@pytest.mark.parametrize("name", ["embed", "frontend", "finetune", "stream"])
def test_committed_bench_line_has_the_contract_fields(name):
    d = _latest_bench_lines()[name]
    for k, t in (("metric", str), ("value", (int, float)), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                 ("ms_per_step", (int, float)), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str),
                 ("config", dict), ("roofline", dict), ("cpu_baseline", dict)):
        assert k in d and isinstance(d[k], t), k
    assert "vs_baseline" in d and d["vs_baseline"] is None            # BASELINE.md publishes no number for this metric
    assert d["scaling"] == "weak" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and "kernel" in r and r["avg_launch_ms"] > 0
    assert r["traffic"] is None or r["traffic"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and isinstance(c["sample"], str)
    # consistency: value = clips per step / step time
    clips = d["config"]["clips_per_gpu"] * d["n_gpus"]
    assert abs(d["value"] - clips / (d["ms_per_step"] * 1e-3)) / d["value"] < 0.01


def test_bench_cli_accepts_the_driver_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup"):
        assert flag in out.stdout


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_multi_gpu_self_spawn_and_refusal(monkeypatch):
    """`python bench.py --gpus N` without a launcher must (a) refuse to report N GPUs from fewer devices and (b) otherwise become
    the launcher the driver uses: torch.distributed.run, one rank per GPU, rendezvous on 127.0.0.1, the original arguments
    passed through, dmabuf IPC left on.  No GPU needed: device count and the process launch are stubbed."""
    import torch
    bench = _load_bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1", "--config", "finetune"])
    args = bench.parse()
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    with pytest.raises(SystemExit) as ei:
        bench.respawn_under_torchrun(args)
    assert "only 1 GPU(s) visible" in str(ei.value.code) and "refusing" in str(ei.value.code)
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 0
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 8)
    monkeypatch.setattr(bench.subprocess, "call", fake_call)
    with pytest.raises(SystemExit) as ei:
        bench.respawn_under_torchrun(args)
    assert ei.value.code == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"] and "--nnodes=1" in cmd and "--nproc-per-node=2" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    tail = cmd[cmd.index(os.path.join(ROOT, "bench.py")) + 1:]
    assert tail == ["--gpus", "2", "--steps", "3", "--warmup", "1", "--config", "finetune"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_launcher_world_size_must_match_gpus(monkeypatch):
    """Under a launcher (WORLD_SIZE set) a mismatching --gpus is an error before any device work... unless there is no GPU at all,
    which is reported first: either way bench.py never prints a line for the wrong world size."""
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode != 0 and "{" not in out.stdout
    assert ("WORLD_SIZE=2" in out.stderr) or ("needs an MI355X" in out.stderr)


def test_dominant_kernel_choice_is_stable_under_timing_noise():
    """Kernels within 5 % of the leader are a tie; the tie goes to the one furthest from its roofline, not to noise."""
    bench = _load_bench()
    pk = {"dense": {"ms": 0.1563, "launches": 3, "flops": 3 * 6.08e9, "bytes": 1e6},
          "pair": {"ms": 0.1537, "launches": 3, "flops": 3 * 4.0e9, "bytes": 1e6},
          "small": {"ms": 0.05, "launches": 1, "flops": 1e8, "bytes": 1e6}}
    r1, _ = bench.roofline_of(pk)
    pk["dense"]["ms"], pk["pair"]["ms"] = 0.1530, 0.1560          # the noise flips the order
    r2, k2 = bench.roofline_of(pk)
    assert r1["kernel"] == r2["kernel"] == "pair" and r1["tied_for_dominant"] == ["dense", "pair"]
    assert 0 < r2["time_weighted_frac"] < 1 and abs(k2["pair"]["frac"] - r2["frac"]) < 1e-3


def test_headline_line_carries_the_other_configs_and_a_sustained_run():
    """Round 6 (verdict item 6): the ONE line `python bench.py --full` prints also holds short runs of the other
    three BASELINE configs (`secondary`, same code path as `--config X`) and a >= 2 s continuation of the headline step (`sustained`: long
    enough for a clock / power sampler to see the GPU busy); `value` stays the K-step figure."""
    d = _latest_bench_lines()["embed"]
    if "secondary" not in d:
        pytest.skip("the committed headline line predates round 6")
    assert d["lanes"] == 1 and "single_stream" not in d                  # one stream: the shipped default (concurrent batches measured, did not pay)
    s = d["sustained"]
    assert s["seconds"] >= 1.9 and s["steps"] >= 50 and s["value"] > 0
    assert abs(s["value"] - d["config"]["clips_per_gpu"] / (s["ms_per_step"] * 1e-3)) / s["value"] < 0.01
    assert abs(s["value"] - d["value"]) / d["value"] < 0.1               # the K-step figure is not a burst artefact
    sec = d["secondary"]
    assert set(sec) == {"frontend", "finetune", "stream"}
    for name, unit in (("frontend", "clips/s"), ("finetune", "clips/s"), ("stream", "windows/s")):
        e = sec[name]
        assert e["value"] > 0 and e["unit"] == unit and e["ms_per_step"] > 0 and 0 < e["whole_step_frac"] < 1, name
        assert e["dominant"]["kernel"] and 0 < e["dominant"]["frac"] < 1
    assert sec["frontend"]["workload"].startswith("configs[1]") and sec["finetune"]["workload"].startswith("configs[3]") and sec["stream"]["workload"].startswith("configs[4]")
    assert sec["stream"]["latency_ms_batch1"] > 0


def test_bench_cli_has_the_round6_switches():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    for flag in ("--lanes", "--sustain-s", "--no-secondary"):
        assert flag in out.stdout


def test_bench_cli_has_full_and_dump_outputs(monkeypatch):
    """A plain run is lean: everything beyond the headline figure sits behind --full (off by default)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    for flag in ("--full", "--dump-outputs"):
        assert flag in out.stdout
    bench = _load_bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and args.steps == 7 and args.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_dump_outputs_writes_float_arrays_under_the_cap(tmp_path, monkeypatch):
    import numpy as np
    bench = _load_bench()
    rng = np.random.default_rng(3)
    arrays = {"emb": rng.standard_normal((64, 32)).astype(np.float32), "wide": rng.standard_normal(10), "count": np.arange(5)}
    shapes = bench.dump_outputs(str(tmp_path / "a"), arrays)
    assert shapes == {"emb": [64, 32], "wide": [10], "count": [5]}
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in arrays}
    assert got["emb"].dtype == np.float32 and np.array_equal(got["emb"], arrays["emb"])
    assert got["wide"].dtype == np.float64 and np.array_equal(got["wide"], arrays["wide"])
    assert got["count"].dtype == np.float32 and np.array_equal(got["count"], np.arange(5, dtype=np.float32))
    # above the cap: a fixed, seeded sample of each array, the same from call to call
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1000)
    s1 = bench.dump_outputs(str(tmp_path / "b"), arrays)
    s2 = bench.dump_outputs(str(tmp_path / "c"), arrays)
    assert s1 == s2 and sum(np.load(tmp_path / "b" / f"{k}.npy").nbytes for k in arrays) <= 1000
    for k in arrays:
        assert np.array_equal(np.load(tmp_path / "b" / f"{k}.npy"), np.load(tmp_path / "c" / f"{k}.npy"))
    assert set(np.load(tmp_path / "b" / "emb.npy").tolist()) <= set(arrays["emb"].reshape(-1).tolist())


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps_the_last_step(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` without --full: exactly K timed steps, the headline fields, none of the --full
    figures; --dump-outputs holds the embeddings of the last step, which a direct forward pass on the same clips reproduces."""
    import numpy as np
    import torch
    from multilingual_kws_amd import synth, weights
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    from multilingual_kws_amd.frontend import Frontend
    d = str(tmp_path / "out")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", d],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    for k, t in (("metric", str), ("value", float), ("unit", str), ("higher_is_better", bool), ("dtype", str), ("ms_per_step", float)):
        assert isinstance(line[k], t), k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False and line["cpu_baseline"] is None
    assert not {"roofline", "kernels", "whole_step", "sustained", "secondary"} & set(line)
    assert abs(line["value"] - 1024 / (line["ms_per_step"] * 1e-3)) / line["value"] < 0.01
    assert line["dumped_outputs"] == {"embeddings": [1024, 1024]}
    got = np.load(os.path.join(d, "embeddings.npy"))
    assert got.dtype == np.float32 and np.isfinite(got).all()
    dev = torch.device("cuda:0")
    audio = torch.from_numpy(synth.clips_float32(1024, first_clip=0)).to(dev)
    ref = EmbeddingModel(weights.synthetic_blob(), max_batch=1024, device=dev).forward(Frontend(max_samples=16000).forward(audio)).cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
