"""CPU: the rectangle an evaluation frame bins (preprocess.hip binned_rect / blend_math.h alpha_box, restated in
tests/alpha_rect_check.py) never drops a tile that holds a pixel the render would accept -- brute force over the pixel
centres of every dropped tile with the render's own float32 accept arithmetic -- and keeps the reference's rectangle
whenever the conic is not a sane ellipse.

What the restatement predicts for the scenes of tests/test_gpu_alpha_rect.py (CPU oracle preprocess; instances of the
reference's rectangles -> of the binned ones):
    opacity_sweep    67201 ->  1569  (0.023)     elongated       156949 -> 82928  (0.528)
    faint           103181 -> 33813  (0.328)     all_empty          820 ->     0
    single              12 ->     6  (0.500)     one_covers_all     151 ->   126  (0.834)
and for the constructed splats of the first test: 0.499 of 687 k instances stay, 344 k dropped tiles are brute-forced.
"""
import numpy as np
import pytest

import alpha_rect_check as ar

f32 = np.float32


@pytest.fixture(scope="module")
def splats():
    return ar.constructed_splats(210_000, seed=7)


def test_no_accepted_pixel_outside_the_binned_rectangle(splats):
    px, py, a, b, c, op, rect = splats
    assert len(px) >= 200_000
    bad, looked = ar.accepted_outside(px, py, a, b, c, op, rect)
    assert looked > 100_000          # dropped tiles that were brute-forced
    assert bad == 0
    # and it is worth something: the share of the reference's instances that stay
    ref = ar.instance_counts(rect).sum()
    bx0, by0, bx1, by1, kept = ar.binned_rect(px, py, a, b, c, op, rect)
    got = (ar.instance_counts((bx0, by0, bx1, by1)) * kept).sum()
    assert 0 < got < 0.9 * ref


def test_binned_rectangle_lies_inside_the_reference_rectangle(splats):
    px, py, a, b, c, op, rect = splats
    bx0, by0, bx1, by1, kept = ar.binned_rect(px, py, a, b, c, op, rect)
    k = kept
    assert (bx0[k] >= rect[0][k]).all() and (bx1[k] <= rect[2][k]).all()
    assert (by0[k] >= rect[1][k]).all() and (by1[k] <= rect[3][k]).all()


def test_transparent_splats_keep_no_tile(splats):
    px, py, a, b, c, op, rect = splats
    kept = ar.binned_rect(px, py, a, b, c, op, rect)[4]
    below = op < f32((1.0 / 255.0) * 0.999)
    assert below.sum() > 1000 and not kept[below].any()
    # from 2/255 on the pixel a centre sits on (within a quarter pixel: q <= 3.4 * 0.125 < 2 ln 2) is accepted, so
    # its tile stays
    tx, ty = np.floor(np.round(px) / 16), np.floor(np.round(py) / 16)
    centre_in = (tx >= rect[0]) & (tx < rect[2]) & (ty >= rect[1]) & (ty < rect[3])
    above = (op >= f32(2.0 / 255.0)) & centre_in & (np.abs(px - np.round(px)) < 0.25) & (np.abs(py - np.round(py)) < 0.25)
    assert above.sum() > 1000 and kept[above].all()


def test_a_conic_that_is_no_sane_ellipse_keeps_the_reference_rectangle():
    nan, inf = f32(np.nan), f32(np.inf)
    rows = [(-1.0, 0.0, 1.0), (1.0, 0.0, -1.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (1.0, 2.0, 1.0), (1.0, 1.0, 1.0),
            (nan, 0.0, 1.0), (1.0, nan, 1.0), (1.0, 0.0, nan), (inf, 0.0, 1.0), (1.0, 0.0, inf), (1.0, inf, 1.0),
            (inf, inf, inf), (1e-30, 0.0, 1e-30), (3e38, 0.0, 3e38)]
    a, b, c = (np.array(v, f32) for v in zip(*rows))
    n = len(rows)
    px = np.full(n, 40.3, f32); py = np.full(n, 30.7, f32)
    rect = ar.reference_rect(px, py, np.full(n, 25), 8, 6)
    for op in (0.9, 0.004, nan, inf):
        o = np.full(n, op, f32)
        bx0, by0, bx1, by1, kept = ar.binned_rect(px, py, a, b, c, o, rect)
        assert kept.all()
        assert (bx0 == rect[0]).all() and (by0 == rect[1]).all() and (bx1 == rect[2]).all() and (by1 == rect[3]).all()
    # ... except below the opacity floor, where no pixel passes whatever the conic
    assert not ar.binned_rect(px, py, a, b, c, np.full(n, 0.5 / 255.0, f32), rect)[4].any()
    # non-finite centres: kept as well
    for bad in (nan, inf, -inf):
        p = np.full(n, bad, f32)
        good = np.full(n, 1.0, f32)
        assert ar.binned_rect(p, py, good, 0 * good, good, np.full(n, 0.9, f32), rect)[4].all()


def test_kept_ratio_of_the_gpu_scenes():
    got = {name: ar.oracle_counts(sc, W, H) for name, (sc, W, H) in ar.scenes().items()}
    for name, (R, B, kept, vis) in got.items():
        print("%-16s instances %6d binned %6d ratio %.3f  visible %5d kept %5d" % (name, R, B, B / max(R, 1), vis, kept))
    R, B, kept, vis = got["faint"]
    assert R > 10_000 and B <= 0.8 * R            # the scene the GPU test uses to show the feature is on
    R, B, kept, vis = got["all_empty"]
    assert vis > 100 and kept == 0 and B == 0
    R, B, kept, vis = got["single"]
    assert vis == 1 and kept == 1
    R, B, kept, vis = got["one_covers_all"]
    assert R >= 7 * 5 and B >= 7 * 5                # 104 x 72: 6.5 x 4.5 tiles, all of them in the big splat's box
    R, B, kept, vis = got["opacity_sweep"]
    assert 0 < kept < vis                            # some of the sweep's splats leave the binning, some stay
    assert 0 < got["elongated"][1] < got["elongated"][0]
