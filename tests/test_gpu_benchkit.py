"""GPU tests of tools/benchkit.py, the timing scaffold the side benches in tools/ share, on a 1024-element tensor: how
often and in what order the timed functions are called, that the device events lie inside the host clock's window, that
each switch leaves its time out, the sync counter and the one-pass kernel list."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import benchkit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def x():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.zeros(1024, dtype=torch.float32, device="cuda:0")


def test_timed_calls_and_samples(x):
    calls = []
    samples = benchkit.timed(lambda: calls.append(x.add_(1)), steps=4, warmup=2)
    assert len(calls) == 6 and len(samples) == 4
    for s in samples:                      # the events are recorded inside the clock's window
        assert 0 < s["device_us"] <= s["wall_us"], s


def test_timed_prepare_feeds_fn(x):
    made, got = [], []

    def prepare():
        made.append(len(made))
        return made[-1]
    samples = benchkit.timed(lambda k: got.append(k) or x.add_(1), steps=4, warmup=2, prepare=prepare)
    assert made == list(range(6)) and got == made and len(samples) == 4


def test_switches_leave_their_time_out(x):
    for s in benchkit.timed(lambda: x.add_(1), steps=4, warmup=2, events=False):
        assert set(s) == {"wall_us"} and s["wall_us"] > 0
    for s in benchkit.timed(lambda: x.add_(1), steps=4, warmup=2, wall=False):
        assert set(s) == {"device_us"} and s["device_us"] > 0
    assert set(benchkit.batch(lambda: x.add_(1), 8, events=False)) == {"wall_us"}
    s = benchkit.batch(lambda: x.add_(1), 8)
    assert 0 < s["device_us"] <= s["wall_us"], s


def test_alternating_takes_turns(x):
    order = []
    routes = {"a": lambda: order.append("a") or x.add_(1), "b": lambda: order.append("b") or x.mul_(1)}
    samples = benchkit.alternating(routes, steps=3, warmup=1)
    assert order == ["a", "b"] * 4
    assert set(samples) == {"a", "b"} and all(len(v) == 3 for v in samples.values())


def test_count_syncs(x):
    assert benchkit.count_syncs(lambda: x.sum().item()) == 1
    assert benchkit.count_syncs(lambda: x.add_(1)) == 0

    def raises():
        raise RuntimeError("inside the counted call")
    with pytest.raises(RuntimeError):
        benchkit.count_syncs(raises)
    assert torch.cuda.get_sync_debug_mode() == 0


def test_device_kernels_lists_the_one_kernel(x):
    try:                        # the tools' "error record" case: the profiler itself does not start here
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]):
            pass
    except Exception as e:
        pytest.skip("torch.profiler is not available: %s: %s" % (type(e).__name__, e))
    kernels = benchkit.device_kernels(lambda: x.add_(1))
    assert len(kernels) == 1, kernels
    assert benchkit.launch_counts(kernels) == {"kernels": 1, "copies_and_memsets": 0}
