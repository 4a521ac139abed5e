"""Host tests of tools/benchkit.py, the timing scaffold the side benches in tools/ share: the parts that touch no device
(the upper median, the repetitions' dict, the one JSON line and its --out file, the rocprofv3 kernel_stats.csv reader,
the refusal without a GPU)."""
import json
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import benchkit


def test_median_is_the_upper_median():
    assert benchkit.median([4, 1, 3, 2]) == 3
    assert benchkit.median([5]) == 5
    rng = random.Random(7)
    for n in (7, 8):
        xs = [rng.random() for _ in range(n)]
        assert benchkit.median(xs) == sorted(xs)[len(xs) // 2]


@pytest.mark.parametrize("unit,prefix,keys", [
    ("us", "wall_", ("wall_us", "wall_min_us", "wall_max_us", "wall_medians_us")),
    ("ms", "", ("ms", "min_ms", "max_ms", "medians_ms"))])
def test_spread_keys(unit, prefix, keys):
    meds = [3.5, 1.25, 2.0, 9.0]
    got = benchkit.spread(list(meds), unit=unit, prefix=prefix)
    assert set(got) == set(keys) and len(got) == 4
    assert [got[k] for k in keys] == [3.5, 1.25, 9.0, meds]


def test_medians_and_column_take_each_time_of_the_samples():
    samples = [{"wall_us": 4.0, "device_us": 1.0}, {"wall_us": 1.0, "device_us": 3.0}, {"wall_us": 3.0, "device_us": 2.0},
               {"wall_us": 2.0, "device_us": 0.5}]
    assert benchkit.column(samples, "wall_us") == [4.0, 1.0, 3.0, 2.0]
    assert benchkit.medians(samples) == {"wall_us": 3.0, "device_us": 2.0}
    assert benchkit.medians([{"device_us": 7.0}]) == {"device_us": 7.0}


def test_windows_take_turns_and_warm_up_once(monkeypatch):
    """per repetition one window per route, in the routes' order; `warmup` calls in front of the first repetition's
    windows, `again` in front of the later ones; the switches reach `timed`; the medians come back repetition by
    repetition"""
    seen = []

    def timed(fn, steps, warmup, **switches):
        seen.append((fn, steps, warmup, switches))
        base = 10.0 * len(seen)
        return [{"device_us": base + x} for x in (3.0, 1.0, 2.0)]
    monkeypatch.setattr(benchkit, "timed", timed)
    got = benchkit.windows({"a": "fa", "b": "fb"}, 3, 5, 4, wall=False)
    assert seen == [(f, 5, w, {"wall": False}) for w in (4, 1, 1) for f in ("fa", "fb")]
    assert got == {"a": {"device_us": [12.0, 32.0, 52.0]}, "b": {"device_us": [22.0, 42.0, 62.0]}}
    del seen[:]
    benchkit.windows({"a": "fa"}, 2, 5, 4, again=2)
    assert [s[2] for s in seen] == [4, 2]


def test_optional_turns_a_raise_into_the_error_record():
    assert benchkit.optional(lambda a, b: a + b, 1, 2) == 3

    def raises():
        raise RuntimeError("no profiler here")
    assert benchkit.optional(raises) == {"error": "RuntimeError: no profiler here"}


def test_launch_counts_sets_copies_and_memsets_apart():
    assert benchkit.launch_counts([]) is None
    kernels = [("void at::native::vectorized_elementwise_kernel<4>", 3.0), ("Memcpy DtoH (Device -> Pinned)", 2.0),
               ("Memset (Device)", 1.0), ("tracks_pose_kernel", 5.0)]
    assert benchkit.launch_counts(kernels) == {"kernels": 2, "copies_and_memsets": 2}


def test_emit_prints_one_line_and_writes_the_indented_document(capsys, tmp_path):
    result = {"bench": "x", "cases": {"a": {"us": 1.5, "medians_us": [1.0, 1.5, 2.0]}}, "kept": 3}
    benchkit.emit(result)
    out = capsys.readouterr().out
    assert out.endswith("\n") and out.count("\n") == 1
    assert json.loads(out) == result
    path = tmp_path / "not" / "yet" / "there.json"
    benchkit.emit(result, str(path))
    assert json.loads(capsys.readouterr().out) == result
    assert path.read_text() == json.dumps(result, indent=1) + "\n"


def test_kernel_stats_reads_the_asked_for_kernels(tmp_path):
    path = tmp_path / "kernel_stats.csv"
    path.write_text('"Name","Calls","TotalDurationNs","AverageNs"\n'
                    '"void nms_candidates_kernel<80>(float const*)",35,70000,2000.5\n'
                    '"nms_walk_kernel(int)",7,21000,3000\n'
                    '"some_other_kernel",9,900,100\n')
    got = benchkit.kernel_stats(str(path), ("nms_candidates_kernel", "nms_walk_kernel"))
    assert got == {"nms_candidates_kernel": {"avg_us": 2000.5 / 1e3, "calls": 35},
                   "nms_walk_kernel": {"avg_us": 3000 / 1e3, "calls": 7}}
    assert all(type(v["calls"]) is int for v in got.values())


def test_require_gpu_refuses_without_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit) as e:
        benchkit.require_gpu("x")
    assert str(e.value).startswith("x: needs an MI355X")
