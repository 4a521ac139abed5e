"""CPU only: the exact-length frames of tests/list_boundary_truth.py are what they claim to be, and the band
comparison the GPU tests apply to the HIP backward is (a) met by the oracle itself and (b) not met by gradients with one
list entry dropped, doubled or a tenth short.

For every case: `conditions` by the oracle's forward alone; the oracle's backward against float64 autograd
(helpers.float64_truth_gradients) band by band; every planted error beyond max(4 err(oracle), FLOOR) in the band it
was planted in, and FLOOR <= 1/10 of the smallest planted figure -- the one constraint on FLOOR that needs no GPU.
Figures are printed before they are asserted and collected in bench_out/list_boundary_host.json (committed copy:
profiles/list_boundary_host.json).
"""
import json
import os

import numpy as np
import pytest
import torch

import list_boundary_truth as lb
from helpers import float64_truth_gradients, gaussians_fed_by_fragile_pixels, oracle_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG = torch.tensor([0.1, 0.4, 0.2])

# How far the oracle itself may lie from float64 in one band: its walk starts from T_final = 1 - alphas[pix] with
# alphas the float32 sum of the weights (helpers.float64_truth_gradients), which on these frames (alpha <= 0.98 after up
# to ~1600 blended terms) is ~1e-4 relative; float32 per-term rounding adds 1e-6.  Two orders below a planted error.
ORACLE_BAND_BAR = 2e-3


def _record(key, value):
    """One case per line: the committed copy stays readable in a diff."""
    out = os.path.join(ROOT, "bench_out")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "list_boundary_host.json")
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[key] = value
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(data[k], sort_keys=True))
                                   for k in sorted(data)) + "\n}\n")


def _sig(x):
    return float("%.3g" % x)


@pytest.mark.parametrize("case", list(lb.CASES))
def test_case_meets_its_conditions_and_planted_errors_are_rejected(case):
    import oracle
    sc, cam = lb.scene(case)
    H, W = cam.image_height, cam.image_width
    o = lb.oracle_forward(sc, cam, BG)
    cond = lb.conditions(case, o)
    print(case, cond)
    g = torch.Generator().manual_seed(7)
    gc, gd, ga = torch.randn(3, H, W, generator=g), 0.1 * torch.randn(1, H, W, generator=g), torch.randn(1, H, W, generator=g)
    ref = lb.oracle_grads(oracle.backward(o, gc, gd, ga))
    truth = float64_truth_gradients(sc, oracle_kwargs(cam, sc.sh_degree, bg=BG), gc, gd, ga)
    exempt = gaussians_fed_by_fragile_pixels(o)
    rows = lb.band_rows(o, exempt)
    assert sum(len(r[3]) for r in rows) == int((lb.is_contributor(o) & ~exempt).sum())
    err = lb.band_errors(ref, truth, o, exempt, rows)
    worst = {k: float(v.max()) for k, v in err.items() if v.size}
    print(case, "oracle against float64, worst band:", worst)
    planted, by_band = [], {}
    for name, i, wrong in lb.planted_errors(ref, o, exempt):
        ids = rows[i][3]
        caught = [k for k in err if lb._rel(wrong[k], truth[k], ids) > lb.band_threshold(err[k][i])]
        planted.append(dict(name=name, figure=lb.planted_figure(wrong, truth, rows, i), caught_by=caught))
        by_band.setdefault(i, []).append(planted[-1])
    smallest = min((p["figure"] for p in planted), default=None)
    print(case, "planted errors: %d, smallest figure %s" % (len(planted), smallest))
    # per planted band: [tile, from, to, dropped, doubled, tenth lost (figures), fewest arrays that caught one]
    _record(case, dict(conditions={k: (_sig(v) if isinstance(v, float) else v) for k, v in cond.items()}, bands=len(rows),
                       oracle_worst_band_error={k: _sig(v) for k, v in worst.items()},
                       planted=[[int(x) for x in rows[i][:3]] + [_sig(p["figure"]) for p in ps] +
                                [min(len(p["caught_by"]) for p in ps)] for i, ps in sorted(by_band.items())],
                       smallest_planted_figure=_sig(smallest), floor=lb.FLOOR))
    assert all(v <= ORACLE_BAND_BAR for v in worst.values()), worst
    assert planted and all(p["caught_by"] for p in planted), [p for p in planted if not p["caught_by"]]
    assert lb.FLOOR <= 0.1 * smallest and lb.WEIGHT_FLOOR <= 0.1 * smallest, (lb.FLOOR, smallest)


@pytest.mark.parametrize("case", ["one_257", "mixed_8193_4096", "blocker_6144"])
def test_blend_weights_in_closed_form(case):
    """colors_precomp and loss = sum of the colour planes: dL_dcolors[g] = sum over pixels of alpha T, every term
    positive.  The oracle's worst relative error per non-exempt contributor against float64 is the yardstick of the GPU
    test; here: it is far below the weight a single (pixel, Gaussian) term carries."""
    import oracle
    sc, cam = lb.scene(case)
    H, W = cam.image_height, cam.image_width
    colors = torch.rand(sc.means3D.shape[0], 3, generator=torch.Generator().manual_seed(3))
    o = lb.oracle_forward(sc, cam, BG, colors=colors)
    z = torch.zeros(1, H, W)
    ref = oracle.backward(o, torch.ones(3, H, W), z, z)
    truth = float64_truth_gradients(sc, oracle_kwargs(cam, sc.sh_degree, bg=BG), torch.ones(3, H, W), z, z, colors=colors)
    keep = lb.is_contributor(o) & ~gaussians_fed_by_fragile_pixels(o)
    w, t = np.asarray(ref["dL_dcolors"], np.float64)[keep], truth["dL_dcolors"][keep]
    assert (t >= 0).all() and np.allclose(t[:, 0], t[:, 1], rtol=1e-12, atol=0) and np.allclose(t[:, 0], t[:, 2], rtol=1e-12, atol=0)
    live = t[:, 0] > 0
    rel = np.abs(w[live] - t[live]).max(1) / t[live, 0]
    print(case, "oracle's worst relative weight error %.2e over %d Gaussians" % (rel.max(), live.sum()))
    _record("weights/" + case, dict(oracle_worst_rel=_sig(rel.max()), gaussians=int(live.sum())))
    assert rel.max() <= 1e-3
