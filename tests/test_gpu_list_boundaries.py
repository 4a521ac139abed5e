"""-m gpu: the render and its backward at every tile-list length where the blend kernels change code path
(tests/list_boundary_truth.py: 64 / 128 / 256 / 2048 / 4096 / every further 2048 / 8192, one entry below, on and above),
on frames whose lists have exactly those lengths.

Forward: test_gpu_forward's _check against the oracle (keys, point list, ranges bit-exact, n_contrib exact off the
fragile pixels, planes within 1e-4), with and without semantic planes.  Backward: test_gpu_backward's _run with the
project's bars, then BAND BY BAND (64 list positions) against float64 autograd: per band and array
err(HIP) <= max(4 err(oracle), FLOOR) -- the oracle is the yardstick, 4 the margin this project gives a fused op over its
float32 yardstick; FLOOR (list_boundary_truth.FLOOR) was set once from the first band-by-band measurement of the HIP
backward and is held under 1/10 of the smallest planted-error figure by tests/test_list_boundary_host.py.  Also: the
blend weights in closed form, the segmented walk against the single-chain walk, two backwards on one forward, sort
binning and an overflowing capacity hint, layered frames with and without object entries in the long tile.

Every GPU test asserts list_boundary_truth.conditions on its own inputs.  Figures are printed before they are asserted
and collected in bench_out/list_boundary_parity.json (committed copy: profiles/list_boundary_parity.json): per case the
worst figure of each array, and for the plain backward every band's worst figure over the arrays, HIP and oracle.
"""
import json
import os

import numpy as np
import pytest
import torch

import list_boundary_truth as lb
import oracle
from helpers import float64_truth_gradients, gaussians_fed_by_fragile_pixels, oracle_kwargs
from test_gpu_backward import _rel_l2, _run, _scene_gradients
from test_gpu_forward import _check, _rasterize
from test_gpu_layers import _check as _layers_equal_three_calls

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG = torch.tensor([0.1, 0.4, 0.2])
CHECKPOINTED = tuple(k for k in lb.BACKWARD if max(lb.CASES[k]["lengths"]) >= 4095)   # 4095: the last list without


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.device("cuda:0")


def _record(key, value):
    """One key per line: the committed copy stays readable in a diff."""
    out = os.path.join(ROOT, "bench_out")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "list_boundary_parity.json")
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[key] = value
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join("%s:%s" % (json.dumps(k), json.dumps(data[k], sort_keys=True, separators=(",", ":")))
                                   for k in sorted(data)) + "\n}\n")


def _worst(rec):
    return {k: dict(hip=max(v["got"], default=0.0), yardstick=max(v["yardstick"], default=0.0))
            for k, v in rec["arrays"].items()}


def _per_band(figures):
    """tile -> {from, hip, oracle}: per band its first list position and its worst figure over the gradient arrays, in
    units of 1e-8 (from = 64 where no band was merged: band i starts at 64 i)."""
    worst = lambda side: np.max([v[side] for v in figures["arrays"].values()], axis=0)   # noqa: E731
    out = {}
    for (t, lo, _, _), h, y in zip(figures["bands"], worst("got"), worst("yardstick")):
        d = out.setdefault(str(t), {"from": [], "hip": [], "oracle": []})
        d["from"].append(lo), d["hip"].append(int(round(h * 1e8))), d["oracle"].append(int(round(y * 1e8)))
    for d in out.values():
        if d["from"] == list(range(0, lb.BAND * len(d["from"]), lb.BAND)):
            d["from"] = lb.BAND
    return out


def _forward(dev, case, S=0):
    sc, cam = lb.scene(case)
    sem = torch.rand(sc.means3D.shape[0], S, generator=torch.Generator().manual_seed(S)) if S else None
    o = lb.oracle_forward(sc, cam, BG, semantics=sem)
    lb.conditions(case, o)
    return sc, cam, sem, o


@pytest.mark.parametrize("case", list(lb.CASES))
def test_forward_at_exact_list_lengths(dev, case):
    sc, cam, _, o = _forward(dev, case)
    _check(_rasterize(dev, sc, cam, bg=BG), o, max_fragile_frac=0.02)


@pytest.mark.parametrize("S", [3, 17])
@pytest.mark.parametrize("case", lb.EDGES + lb.MIXED)
def test_forward_with_semantic_planes(dev, case, S):
    """S > 0: every list takes the heavy path (heavy_min = 1), the wave pairs carry the planes through the MFMA, and
    channel 16 of S = 17 comes from the stand-alone kernel."""
    sc, cam, sem, o = _forward(dev, case, S)
    got = _rasterize(dev, sc, cam, bg=BG, semantics=sem)
    assert got["semantic"].shape == (S, cam.image_height, cam.image_width)
    _check(got, o, max_fragile_frac=0.02)


def _record_now(key, per_band):
    """assert_bands hands its figures over BEFORE it asserts."""
    def rec(figures):
        out = dict(worst=_worst(figures), floor=lb.FLOOR)
        if per_band:
            out.update(bands_1e8=_per_band(figures))
        _record(key, out)
    return rec


@pytest.mark.parametrize("case", lb.BACKWARD)
def test_backward_band_by_band(dev, case):
    """_run with the project's own bars (float64 autograd as the arbiter), then every band of every gradient array."""
    sc, cam = lb.scene(case)
    r = _run(dev, sc, cam, BG, seed=5, with_truth=True)
    lb.conditions(case, r["o"])
    key = "backward/" + case
    lb.assert_bands(key, r["hip"], lb.oracle_grads(r["ref"]), r["truth"], r["o"], r["exempt"],
                    record=_record_now(key, True))


@pytest.mark.parametrize("case", lb.BACKWARD)
def test_blend_weights_in_closed_form(dev, case):
    """colors_precomp, loss = sum of the colour planes: dL_dcolors[g] = sum over pixels of alpha T; every term is
    positive, nothing cancels, and the smallest single term is >~ 1e-3 of its sum.  Per non-exempt contributor the HIP
    weight lies within max(4 x the oracle's own worst figure on this case, WEIGHT_FLOOR) of float64."""
    sc, cam = lb.scene(case)
    H, W = cam.image_height, cam.image_width
    colors = torch.rand(sc.means3D.shape[0], 3, generator=torch.Generator().manual_seed(3))
    o = lb.oracle_forward(sc, cam, BG, colors=colors)
    lb.conditions(case, o)
    one, z = torch.ones(3, H, W), torch.zeros(1, H, W)
    ref = oracle.backward(o, one, z, z)
    truth = float64_truth_gradients(sc, oracle_kwargs(cam, sc.sh_degree, bg=BG), one, z, z, colors=colors)
    hip = _scene_gradients(dev, sc, cam, BG, (one, z, z), colors=colors)[0][2]
    keep = lb.is_contributor(o) & ~gaussians_fed_by_fragile_pixels(o)
    t = truth["dL_dcolors"][keep]
    live = t[:, 0] > 0
    rel = lambda a: np.abs(np.asarray(a, np.float64)[keep][live] - t[live]).max(1) / t[live, 0]   # noqa: E731
    e_hip, e_or = rel(hip), rel(ref["dL_dcolors"])
    print("%s: worst relative weight error HIP %.3e, oracle %.3e, %d Gaussians" % (case, e_hip.max(), e_or.max(), live.sum()))
    _record("weights/" + case, dict(hip=float("%.3g" % e_hip.max()), oracle=float("%.3g" % e_or.max()), gaussians=int(live.sum()),
                                    floor=lb.WEIGHT_FLOOR))
    assert live.sum() >= 4          # (a cut image leaves contributors centred outside it without a weight)
    assert e_hip.max() <= max(4.0 * e_or.max(), lb.WEIGHT_FLOOR), (case, int(np.argmax(e_hip)), e_hip.max(), e_or.max())


_NAMES = ("dL_dmeans3D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations", "dL_dmeans2D_xy")


def _named(grads):
    d = dict(zip(_NAMES, grads))
    d["dL_dmeans2D_xy"] = d["dL_dmeans2D_xy"][:, :2]
    return d


def _planes(cam, seed=5):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(c, cam.image_height, cam.image_width, generator=g) for c in (3, 1, 1))


@pytest.mark.parametrize("case", CHECKPOINTED)
def test_segments_match_single_chain_band_by_band(dev, case):
    """The segmented walk (blend checkpoints) against the single-chain walk of the same lists (one semantic channel
    the loss ignores: such a frame leaves no checkpoints), with NO exemptions -- both read the same forward and make
    the same accept decisions.  Yardstick: the chain walk run twice (two atomic orders)."""
    sc, cam = lb.scene(case)
    o = lb.oracle_forward(sc, cam, BG)
    lb.conditions(case, o)
    planes = _planes(cam)
    seg = _named(_scene_gradients(dev, sc, cam, BG, planes)[0])
    chain = [_named(_scene_gradients(dev, sc, cam, BG, planes, with_semantic_plane=True)[0]) for _ in range(2)]
    none = np.zeros(sc.means3D.shape[0], bool)
    key = "segments/" + case
    lb.assert_bands(key, seg, chain[1], chain[0], o, none, record=_record_now(key, False))


@pytest.mark.parametrize("case", lb.ZERO_SLACK + lb.BLOCKER)
def test_backward_twice_on_one_forward(dev, case):
    """The checkpoints and (tile, segment) items are state of the frame: a second backward finds them unchanged --
    band by band within FLOOR of the first (only the float atomics' order differs)."""
    sc, cam = lb.scene(case)
    o = lb.oracle_forward(sc, cam, BG)
    lb.conditions(case, o)
    g1, g2 = _scene_gradients(dev, sc, cam, BG, _planes(cam), backward_twice=True)
    for a, b in zip(g1, g2):
        assert np.isfinite(a).all() and _rel_l2(a, b) < 1e-5
    none = np.zeros(sc.means3D.shape[0], bool)
    err = lb.band_errors(_named(g2), _named(g1), o, none)
    worst = {k: float("%.3g" % v.max()) for k, v in err.items()}
    print(case, "second backward against the first, worst band:", worst)
    _record("twice/" + case, worst)
    assert all(v <= lb.FLOOR for v in worst.values()), worst


@pytest.mark.parametrize("path", ["sort_binning", "overflow"])
@pytest.mark.parametrize("case", lb.ZERO_SLACK + lb.MIXED + lb.PARTIAL)
def test_schedules(dev, case, path):
    """Sort binning (another blob layout in front of the checkpoints) and a binning blob promised too little, so that
    the checkpoints come from the re-run tail: forward and band-by-band backward as above."""
    from gaussianrpg_amd.rasterizer import _C
    alg = _C.get_binning_algorithm()
    try:
        if path == "sort_binning":
            _C.set_binning_algorithm(0)
        sc, cam, _, o = _forward(dev, case)

        def hint():     # consumed by the next forward of this (P, W, H)
            if path == "overflow":
                _C.set_capacity_hint(sc.means3D.shape[0], cam.image_width, cam.image_height, 3000, 3000)
        hint()
        _check(_rasterize(dev, sc, cam, bg=BG), o, max_fragile_frac=0.02)
        hint()
        key = "%s/%s" % (path, case)
        r = _run(dev, sc, cam, BG, seed=5, with_truth=True)
        lb.assert_bands(key, r["hip"], lb.oracle_grads(r["ref"]), r["truth"], r["o"], r["exempt"],
                        record=_record_now(key, False))
    finally:
        _C.set_binning_algorithm(alg)
        _C.reset_capacity_hints()


@pytest.mark.parametrize("objects", ["tenth_flagged", "none_flagged"])
@pytest.mark.parametrize("case", lb.LAYERED)
def test_layered_frames(dev, case, objects):
    """LAYERS_PC_MIN = 4096 and RENDER_PC_MIN = 8192 in a layered frame, with object entries in the long tile (one walk
    per layer from 4096 on) and without: the one-call layers frame equals the three calls bit for bit."""
    sc, cam, _, o = _forward(dev, case)
    flags = lb.object_flags(o, 0.1 if objects == "tenth_flagged" else 0.0, seed=1)
    assert int(flags.sum()) == (int(round(0.1 * lb.is_contributor(o).sum())) if objects == "tenth_flagged" else 0)
    _layers_equal_three_calls(dev, sc, torch.from_numpy(flags), cam.image_width, cam.image_height)
