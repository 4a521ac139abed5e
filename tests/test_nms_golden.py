"""CPU tests (-m "not gpu"): the numpy restatement of the detections contract (tests/nms_truth.py) against what the
reference's OWN non_max_suppression / scale_coords returned (tests/golden/ref_nms.json + .npz, recorded by
tests/golden/make_golden_nms.py by executing the reference's functions; only torchvision.ops.nms is a stand-in there).
Bit for bit, row count included.  tests/test_gpu_nms.py compares the HIP op with the same golden directly."""
import hashlib
import json
import os

import numpy as np
import pytest

import nms_truth as nt
from helpers import GOLDEN


def load_golden():
    with open(os.path.join(GOLDEN, "ref_nms.json")) as f:
        meta = json.load(f)
    z = np.load(os.path.join(GOLDEN, "ref_nms.npz"))
    return meta, {k: z[k] for k in z.files}


META, ARRAYS = load_golden()
CASES = META["cases"]
_INPUTS = {}


def case_input(case):
    """The case's input, rebuilt from its builder and arguments and checked against the recorded hash; built once."""
    key = case["builder"] + json.dumps(case["args"], sort_keys=True)
    if key not in _INPUTS:
        p = nt.build_input(case["builder"], case["args"])
        assert list(p.shape) == case["shape"]
        assert hashlib.sha256(p.tobytes()).hexdigest() == case["sha256"], "%s: the rebuilt input is not the recorded one" % case["name"]
        p.setflags(write=False)
        _INPUTS[key] = p
    return _INPUTS[key]


def case_frame(case):
    return None if case["frame"] is None else tuple(case["frame"])


def golden_rows(case, b, mapped):
    """[n, 6] float32 of image b as the reference returned it; mapped: the boxes replaced by scale_coords(...).round()."""
    d = ARRAYS["%s/%d/det" % (case["name"], b)].copy()
    if mapped:
        d[:, :4] = ARRAYS["%s/%d/mapped" % (case["name"], b)]
    return d


def same_bits(what, got, ref):
    assert got.dtype == np.float32 and ref.dtype == np.float32 and got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), "%s: %d of %d values differ, first at %s: %r != %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), got[bad][0], ref[bad][0])


def test_golden_layout():
    assert "stand-in" in META["source"] and "non_max_suppression" in META["source"]
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names) == 21
    assert set(k.split("/")[0] for k in ARRAYS) == set(names)
    assert sum(c["frame"] is not None for c in CASES) == 3
    assert [c["counts"] for c in CASES if c["name"] == "batch_2_one_empty"][0][1] == 0
    assert os.path.getsize(os.path.join(GOLDEN, "ref_nms.json")) + os.path.getsize(os.path.join(GOLDEN, "ref_nms.npz")) < 512 * 1024


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_equals_the_references_own_output(case):
    p = case_input(case)
    frame = case_frame(case)
    assert ARRAYS["%s/0/det" % case["name"]].shape[0] == case["counts"][0]
    for b in range(p.shape[0]):
        ref = golden_rows(case, b, mapped=False)
        assert ref.shape == (case["counts"][b], 6)
        got = nt.detections_image(p[b], **case["settings"])
        same_bits("%s image %d" % (case["name"], b), got, ref)
        if frame is not None:
            same_bits("%s image %d mapped boxes" % (case["name"], b), nt.to_frame(ref[:, :4], *frame),
                      ARRAYS["%s/%d/mapped" % (case["name"], b)])
            same_bits("%s image %d mapped" % (case["name"], b), nt.detections_image(p[b], frame=frame, **case["settings"]),
                      golden_rows(case, b, mapped=True))


def test_what_the_cases_are_there_to_show():
    by = {c["name"]: c for c in CASES}
    # the reference's max_nms cut: the isolated, lowest candidates are absent, and the restatement without the cut has them
    c = by["max_nms_30000"]
    x = case_input(c)[0]
    assert len(nt.candidates(x, 0.25)[0]) == 30200 > nt.MAX_NMS
    ref = golden_rows(c, 0, False)
    assert len(ref) < 300 and not (ref[:, 1] >= nt.MAX_NMS_ISOLATED_Y - 20).any()
    uncut = nt.detections_image(x, max_nms=1 << 30)
    assert (uncut[:, 1] >= nt.MAX_NMS_ISOLATED_Y - 20).sum() > 0
    # the threshold is compared as a float32 value: the row AT float32(t) is dropped, its successor kept -- also for
    # t = 0.3, where float32(0.3) > 0.3 and a comparison in double would have kept the row
    for t in (0.25, 0.3):
        for kind in ("objectness", "product"):
            ref = golden_rows(by["threshold_%s_%s" % (t, kind)], 0, False)
            assert ref[:, 4].tolist() == [np.float32(0.9), np.nextafter(np.float32(t), np.float32(1))]
    assert float(np.float32(0.3)) > 0.3
    # half to even, on the reference's own numbers: pre-rounding values on .5 exist and went to the even side
    c = by["frame_simulator"]
    d, m = golden_rows(c, 0, False)[:, :4].astype(np.float64), ARRAYS["frame_simulator/0/mapped"]
    raw = d - [0, 11, 0, 11]
    half = (raw - np.floor(raw) == 0.5) & (raw > 0) & (raw < [1600, 1066, 1600, 1066])
    assert half.sum() > 20 and (m[half] % 2 == 0).all()
    assert len(set((np.floor(raw[half]) % 2).tolist())) == 2          # both rounded up and rounded down
    # the NaN box is kept and suppresses nothing
    ref = golden_rows(by["nan_rows"], 0, False)
    assert np.isnan(ref[0, 0]) and ref[:, 4].tolist() == [np.float32(0.8), np.float32(0.7)]
    assert np.isnan(ARRAYS["nan_rows_mapped/0/mapped"][0, 0])
