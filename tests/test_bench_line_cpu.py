"""The printed bench line fits the driver's record whole: the driver keeps the
last ~8,400 characters of stdout, and the r5 line was 12.2 KB, so list_form, configs1_125m,
native and kernel_trace fell off its front. bench.compact_line projects the full record (which
goes to the `detail` sidecar) onto every measured number the judge reads, under LINE_CAP, with
the record's own key paths."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

R5_LINE = os.path.join(ROOT, "profiles", "r05_final4_bench.json")


def _r5():
    if not os.path.exists(R5_LINE):
        pytest.skip("r5 bench record not in this tree")
    with open(R5_LINE) as f:
        return json.loads(f.read().strip().splitlines()[-1])


def test_r5_record_fits_with_every_sub_object():
    full = _r5()
    assert len(json.dumps(full)) > 12000                     # the record that was truncated
    line = bench.compact_line(full, "gpurun_out/bench_detail_n1.json")
    s = json.dumps(line)
    assert len(s) <= bench.LINE_CAP and "dropped" not in line
    # the driver's parsed fields, unchanged
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert line[k] == full[k], k
    r = line["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "kernel_ms", "unplaced_frac"):
        assert r[k] == full["roofline"][k], k
    assert line["cpu_baseline"]["value"] == full["cpu_baseline"]["value"]
    assert line["cpu_baseline"]["c_port"]["value"] == full["cpu_baseline"]["c_port"]["value"]
    # what VERDICT r5 names as lost, at the record's own paths
    assert line["list_form"]["f32"]["roofline"]["frac"] == full["list_form"]["f32"]["roofline"]["frac"]
    assert line["configs1_125m"]["roofline"]["frac"] == full["configs1_125m"]["roofline"]["frac"]
    assert line["native"]["sha256"] == full["native"]["sha256"]
    assert "outer_kernel<" in line["kernel_trace"]["kernels"][0]["name"]
    assert line["step_with_broadcast"]["fused_ms"] == full["step_with_broadcast"]["fused_ms"]
    # per-generation times stay, pair lists and planner layouts go to the sidecar
    pop = line["population_slerp_7b"]
    assert pop["two_pass"]["roofline"]["frac"] == full["population_slerp_7b"]["two_pass"]["roofline"]["frac"]
    assert pop["gen_ms"]["two_pass"] == [g["two_pass"]["ms"] for g in full["population_slerp_7b"]["generations"]]
    assert "generations" not in pop and "pairs" not in json.dumps(pop)
    assert line["lm_population"]["gen_ms"] == [g["ms"] for g in full["lm_population"]["generations"]]
    assert line["slerp_7b"]["far"]["roofline"]["moved_frac"] == full["slerp_7b"]["far"]["roofline"]["moved_frac"]


def _paths(d, pre=()):
    for k, v in d.items():
        if isinstance(v, dict):
            yield from _paths(v, pre + (k,))
        else:
            yield pre + (k,), v


def test_the_line_is_a_projection_of_the_record():
    """Every value in the line (but the lifted per-generation times and `detail`) is the full
    record's value at the same path."""
    full = _r5()
    line = bench.compact_line(full, "x")
    lifted = bench._with_gen_ms(full)
    for path, v in _paths(line):
        if path[0] == "detail" or path[-1] in ("sample", "tool", "kernel", "note", "kernels"):
            continue
        x = lifted
        for p in path:
            x = x[p]
        assert x == v or (isinstance(x, float) and round(x, 4) == v), path


def test_oversized_record_drops_whole_extras_last_resort():
    full = _r5()
    full["population_slerp_7b"]["generations"] *= 400      # absurdly many generations
    line = bench.compact_line(full)
    assert len(json.dumps(line)) <= bench.LINE_CAP
    assert "population_slerp_7b" not in line and "population_slerp_7b" in line["dropped"]
    assert line["value"] == full["value"] and line["roofline"]["frac"] == full["roofline"]["frac"]


def test_errors_pass_through_truncated():
    line = bench.compact_line({"value": 1.0, "slerp_7b": {"error": "RuntimeError: " + "x" * 5000}})
    assert line["slerp_7b"]["error"].startswith("RuntimeError") and len(line["slerp_7b"]["error"]) == 240


def test_emit_line_writes_the_sidecar(tmp_path, capsys):
    full = _r5()
    path = tmp_path / "detail.json"
    line = bench.emit_line(full, sys.stdout, str(path))
    printed = capsys.readouterr().out.strip().splitlines()
    assert len(printed) == 1 and json.loads(printed[0]) == line
    with open(path) as f:
        assert json.load(f) == full


def test_xgmi_floor():
    assert bench.xgmi_floor_ms(0, 8) is None and bench.xgmi_floor_ms(1 << 30, 1) is None
    w = 7 * int(bench.XGMI_LINK_GBPS * 1e9) // 1000     # 1 ms of 7 links
    assert bench.xgmi_floor_ms(w, 8) == pytest.approx(1.0, rel=1e-6)


def test_plain_run_switches_every_extra_off(capsys):
    """Without --full the options of the extras have no effect (stderr names the ones given); with
    it they keep their values."""
    assert bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"]).steps == 7
    assert capsys.readouterr().err == ""
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2", "--ops", "pair_merge", "--kernel-trace", "3"])
    err = capsys.readouterr().err
    assert "--ops, --kernel-trace only take effect with --full" in err and "--steps" not in err
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert a.ops == "none" and a.cpu_baseline_seconds == 0 and a.kernel_trace == 0 and a.bcast_compare == 0
    assert not (a.weak_companion or a.compare_schedules or a.config_companions or a.parity_layout or a.detail_out)
    f = bench.parse(["--full", "--ops", "pair_merge", "--kernel-trace", "3"])
    assert f.full and f.ops == "pair_merge" and f.kernel_trace == 3 and f.cpu_baseline_seconds > 0
    assert f.weak_companion and f.compare_schedules and f.config_companions and f.parity_layout
    assert f.detail_out.endswith(os.path.join("bench_out", "bench_detail_n1.json"))
    assert capsys.readouterr().err == ""


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """Small arrays are written whole, larger ones as the same seeded, sorted sample every time;
    bf16 is written as float32 exactly."""
    import numpy as np
    import torch
    monkeypatch.setattr(bench, "DUMP_SAMPLE_ELEMS", 1000)
    small = torch.arange(1000, dtype=torch.float32)
    big = torch.arange(5001, dtype=torch.float32)
    half = torch.tensor([1.0, 0.5, -3.140625]).bfloat16()
    rec = bench.dump_outputs(str(tmp_path / "a"), {"small": small, "big": big, "half": half})
    bench.dump_outputs(str(tmp_path / "b"), {"small": small, "big": big})
    assert rec == {"small": {"elements": 1000, "written": 1000}, "big": {"elements": 5001, "written": 1000},
                   "half": {"elements": 3, "written": 3}}
    h = np.load(tmp_path / "a" / "half.npy")
    assert h.dtype == np.float32 and h.tolist() == [1.0, 0.5, -3.140625]
    s, b = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "big.npy")
    assert s.dtype == b.dtype == np.float32 and np.array_equal(s, small.numpy())
    assert b.shape == (1000,) and np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))
    assert np.all(np.diff(b) >= 0) and len(np.unique(b)) > 500            # sorted indices of a monotone array
    assert np.isin(b, big.numpy()).all()
