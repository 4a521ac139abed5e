"""CPU tests (-m "not gpu"): the float32 restatement of the tracklet -> actor-pose step (tests/tracks_truth.py) equals
what the reference's own methods returned (tests/golden/ref_tracks.*, written by tests/golden/make_golden_tracks.py from
lib/models/actor_pose.py and lib/utils/general_utils.py) bit for bit: translation, rotation, both validation paths,
the fallback when fewer than two camera stamps lie inside the track, and the world pose after the ego product.  The
slerp inside is the stand-in of DESIGN.md section 21 on both sides: roma's float32 bits are not pinned."""
import json
import os

import numpy as np
import pytest
import torch

import tracks_truth as tt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load():
    with open(os.path.join(GOLDEN, "ref_tracks.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "ref_tracks.npz"))


META, ARRAYS = _load()


def test_the_fixture_says_what_it_is():
    assert "stand-in" in META["source"] and "the one step not executed from the reference" in META["source"]
    names = [c["name"] for c in META["cases"]]
    for want in ("plain", "validation_camera_stamps", "validation_fallback", "opt_track_off", "branches", "same_side"):
        assert want in names
    assert all(v.dtype == np.float32 for v in ARRAYS.values())


@pytest.mark.parametrize("row", META["cases"], ids=[c["name"] for c in META["cases"]])
def test_restatement_equals_the_reference_bit_for_bit(row):
    case = tt.build_case(row["builder"], row["args"])
    assert case.sha256() == row["sha256"], "the builder no longer makes the input the fixture was recorded on"
    opt = (None, None) if row["opt_seed"] is None else tt.opt_arrays(case, row["opt_seed"])
    truth = tt.Truth(case, *opt, dtype=torch.float32)
    ts = [tt.BASE + 0.1 * q for q in row["queries"]]
    got = {k: [] for k in ("rot", "trans", "obj_rot", "obj_trans")}
    active = []
    with torch.no_grad():
        for k, t in enumerate(ts):
            ego = tt.ego_pose(k % 4)
            for a, track_id in enumerate(case.ids):
                info = case.obj_info[track_id]
                on = info['start_timestamp'] <= t <= info['end_timestamp']
                active.append(int(on))
                if not on:
                    continue
                rot, trans, _ = truth.tracking(a, t, row["is_val"], row["cam"])
                obj_rot, obj_trans, _ = truth.world(a, t, ego, row["is_val"], row["cam"])
                for key, v in (("rot", rot), ("trans", trans), ("obj_rot", obj_rot), ("obj_trans", obj_trans)):
                    got[key].append(v.numpy())
    assert active == row["active"]
    for key, v in got.items():
        want = ARRAYS["%s/%s" % (row["name"], key)]
        have = np.stack(v)
        assert have.dtype == np.float32 and have.shape == want.shape
        bad = have.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), "%s / %s: %d of %d values differ, first %r != %r" % (
            row["name"], key, int(bad.sum()), bad.size, have[bad][0], want[bad][0])


def test_validation_paths_differ_where_they_should():
    plain, stamps, fallback = (ARRAYS["%s/obj_rot" % n] for n in ("plain", "validation_camera_stamps", "validation_fallback"))
    assert np.array_equal(plain, fallback) and not np.array_equal(plain, stamps)
    assert np.array_equal(ARRAYS["opt_track_off/obj_rot"], ARRAYS["opt_track_off_is_val/obj_rot"])
