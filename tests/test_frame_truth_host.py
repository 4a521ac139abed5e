"""CPU tests (-m "not gpu") of tests/frame_truth.py: the conditions on the frames the GPU tests compare (asserted on the
oracle alone, so that a comparison cannot pass by hiding everything), and the teeth of compare_bytes -- it accepts the
oracle's own bytes and rejects each of five planted faults."""
import numpy as np
import pytest

import frame_truth as ft
from oracle import sky_torch as st

PLAIN = [(200, 136, True), (203, 121, False)]


@pytest.mark.parametrize("W,H,truncate", PLAIN)
@pytest.mark.parametrize("turned", [False, True], ids=["trajectory", "turned"])
def test_conditions_of_the_plain_frames(W, H, truncate, turned):
    c = ft.plain_case(W, H, truncate, turned=turned)
    assert c["ref8"].shape == (H, W, 3) and c["ref8"].dtype == np.uint8 and c["v"].shape == (3, H, W)
    ft.assert_conditions("%dx%d" % (W, H), ft.conditions(c["o"], c["v"], truncate))


def test_conditions_of_the_white_and_the_composed_frame():
    c = ft.plain_case(200, 136, True, fill=1.0)
    ft.assert_conditions("white", ft.conditions(c["o"], c["v"], True))
    # the fill shows: where the mask is off the white fill is composited, not the black one
    assert np.abs(c["v"] - ft.plain_case(200, 136, True)["v"]).max() > 0
    c = ft.composed_case()
    ft.assert_conditions("composed", ft.conditions(c["o"], c["v"], True))
    nb = c["models"][0].xyz.shape[0]
    assert int((c["o"]["radii"][nb:] > 0).sum()) > 500, "the actors must be in view"


def _planted(c, fault):
    o, v, truncate = c["o"], c["v"], c["truncate"]
    H, W = v.shape[1:]
    if fault == "channels reversed":
        return c["ref8"][:, :, ::-1]
    if fault == "shifted one pixel in x":
        return np.roll(c["ref8"], 1, axis=1)
    if fault == "rounded where truncation was asked":
        return ft.to_bytes(v, not truncate)
    color = np.clip(np.asarray(o["color"], np.float64), 0.0, 1.0)
    if fault == "untransposed rotation in the sky's rays":
        w2c = c["w2c"].clone()
        w2c[:3, :3] = c["w2c"][:3, :3].t()
        sky = st.sky_color(c["cube"], c["K"], w2c, H, W, acc=o["alpha"], fill=c["fill"])
        return ft.to_bytes(st.composite(color, o["alpha"], sky, clamp=True), truncate)
    if fault == "acc as the sky weight":
        sky = st.sky_color(c["cube"], c["K"], c["w2c"], H, W, acc=o["alpha"], fill=c["fill"])
        return ft.to_bytes(np.clip(color + sky * np.asarray(o["alpha"], np.float64), 0.0, 1.0), truncate)
    raise KeyError(fault)


FAULTS = ["channels reversed", "shifted one pixel in x", "rounded where truncation was asked",
          "untransposed rotation in the sky's rays", "acc as the sky weight"]


@pytest.mark.parametrize("W,H,truncate", PLAIN)
def test_compare_bytes_accepts_the_clean_frame_and_rejects_each_fault(W, H, truncate):
    c = ft.plain_case(W, H, truncate, turned=True)      # the turned camera: a transposed rotation is another rotation
    s = ft.compare_bytes(c["ref8"], c["v"], c["fragile"], truncate)
    assert s["frac_diff_gt0"] == 0.0 and s["frac_diff_gt1"] == 0.0 and s["pixels"] == H * W * 3
    for fault in FAULTS:
        with pytest.raises(AssertionError, match="beyond their bar"):
            ft.compare_bytes(_planted(c, fault), c["v"], c["fragile"], truncate, name=fault)


def test_compare_bytes_bars_byte_by_byte():
    """One step off is accepted only on a near byte, two steps only on a fragile pixel."""
    c = ft.plain_case(200, 136, True)
    v, frag = c["v"], c["fragile"]
    near = ft.near_boundary(v, True)
    fr = np.broadcast_to(frag[:, :, None], near.shape)

    def moved(where, by):
        y, x, ch = np.argwhere(where)[0]
        g = c["ref8"].copy()
        g[y, x, ch] = g[y, x, ch] + by if g[y, x, ch] + by <= 255 else g[y, x, ch] - by
        return g
    ft.compare_bytes(moved(near & ~fr, 1), v, frag, True)
    ft.compare_bytes(moved(fr & ~near, 2), v, frag, True)
    for where, by in ((~near & ~fr, 1), (near & ~fr, 2), (fr, 4)):      # the fragile bar is 2 or 3 steps, by |v|
        with pytest.raises(AssertionError, match="beyond their bar"):
            ft.compare_bytes(moved(where, by), v, frag, True)
    with pytest.raises(AssertionError):
        ft.compare_bytes(c["ref8"].astype(np.float32), v, frag, True)
