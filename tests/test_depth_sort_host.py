"""No GPU: the crafted key scenes of tests/depth_sort_truth.py are what they claim to be.

The GPU tests (tests/test_gpu_depth_sort.py) compare the HIP depth sort and tile partition with a numpy lexsort on
inputs placed ON the seams of csrc/sort.hip.  That only means something while (1) the constants the inputs are built
from are the kernels', (2) every scene really is its key set -- the CPU oracle agrees with the numpy truth on it --,
(3) every case still has the property it stands for, and (4) the comparison rejects the mistakes a seam bug makes.
All four are asserted here, so a case that stops exercising its seam fails on the host instead of passing silently
on the device.

The 4 M cases are built at full size here too: scene plus oracle binning cost about 3.5 s each.
"""
import os
import re

import numpy as np
import pytest

import depth_sort_truth as dt
from depth_sort_truth import C

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaussianrpg_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_are_the_kernels():
    src = _read("common.h")

    def const(name, kind=r"(?:int|uint32_t)"):
        m = re.search(r"constexpr %s %s = ([^;]+);" % (kind, name), src)
        assert m, name
        return m.group(1).strip()

    ds_threads = int(const("DS_THREADS"))
    assert const("DS_ITEMS") == "8192 / DS_THREADS" and const("DS_CHUNK") == "DS_THREADS * DS_ITEMS"
    assert dt.DS_CHUNK == ds_threads * (8192 // ds_threads) == 8192
    assert dt.DS_BITS == int(const("DS_BITS"))
    assert dt.DS_MAX_CHUNKS == int(const("DS_MAX_CHUNKS"))
    assert const("RS_CHUNK") == "RS_THREADS * RS_ITEMS"
    assert dt.RS_CHUNK == int(const("RS_THREADS")) * int(const("RS_ITEMS"))
    assert dt.CULLED_KEY == int(const("CULLED_KEY").rstrip("u"), 16)
    # key_base and the range decision are expressions of sort.hip, not named constants; the header documents them
    assert "rounded down to 2^18" in src
    sort = _read("sort.hip")
    assert "mn & ~((1u << (2 * DS_BITS)) - 1u)" in sort and "((mx - kbase) >> (3 * DS_BITS)) != 0u" in sort
    assert dt.KEY_ALIGN == 1 << (2 * dt.DS_BITS) and dt.NEAR_SPAN == 1 << (3 * dt.DS_BITS)
    assert "nchunks_ds <= DS_MAX_CHUNKS" in _read("api.hip")
    assert dt.BASE == 0x40000000 and dt.BASE % dt.KEY_ALIGN == 0


def test_the_fourth_pass_digits_floats_reach():
    """Bits [27, 32) of key - key_base over depths 0.21 .. 2^60: the digits 0 .. 3, and no positive finite float
    visible past the near plane (z > 0.2) can reach a digit beyond 8."""
    top = (dt.KEY_2P60 - (dt.KEY_021 & ~(dt.KEY_ALIGN - 1))) >> (3 * dt.DS_BITS)
    assert tuple(range(top + 1)) == dt.PASS3_DIGITS == (0, 1, 2, 3)
    assert (dt.bits(np.finfo(np.float32).max) - (dt.bits(0.2) & ~(dt.KEY_ALIGN - 1))) >> (3 * dt.DS_BITS) == 8
    # and the case's largest key is still a depth inside the deep range
    assert dt.KEY_021 + (3 << 27) <= dt.KEY_2P60


# ----------------------------------------------------------------------------------------------------------------
# claims: one checker per claim name; a claim without a checker fails
# ----------------------------------------------------------------------------------------------------------------
def _chunk_visible(visible, c):
    return visible[c * C:(c + 1) * C]


def _claim_dead_chunks(v, x):
    n = -(-x["P"] // C)
    for c in range(n):
        assert _chunk_visible(x["visible"], c).any() == (c not in v), c
    assert all(c < n for c in v)


def _claim_straddle(v, x):
    seams = list(range(C, x["P"], C))
    assert v and seams
    for s in seams:
        assert x["visible"][s - 1] and x["visible"][s] and x["keys"][s - 1] == x["keys"][s], s


def _claim_runs(run, x):
    keys, P = x["keys"].astype(np.int64), x["P"]
    blocks = [keys[b:b + run] for b in range(0, P, run)]
    assert len(blocks) >= 4 and all(np.unique(b).size == 1 for b in blocks)
    first = np.array([b[0] for b in blocks])
    assert (first[1:] != first[:-1]).all() and first[0] > first[1]


def _claim_only_digit(p, x):
    vis = x["keys"][x["visible"]]
    for q in range(4):
        d = np.unique(dt.digits(vis, x["e"]["key_base"], q))
        if q == p:
            assert tuple(d.tolist()) == tuple(x["claims"]["digit_values"]), (q, d)
        else:
            assert d.size == 1, (q, d)


def _claim_far_if_culled_counted(v, x):
    everything = dt.expected(x["keys"], x["tile"], np.ones(x["P"], bool), x["gx"], x["gy"])
    assert v and everything["far"] and not x["e"]["far"]
    ck = x["keys"][~x["visible"]]
    assert ck.size and ((ck < x["e"]["min_key"]) | (ck > x["e"]["max_key"])).all()


def _claim_tiles(T, x):
    assert x["gx"] * x["gy"] == T == x["e"]["ranges"].shape[0]
    lens = x["e"]["ranges"][:, 1].astype(np.int64) - x["e"]["ranges"][:, 0]
    assert lens.sum() == x["e"]["V"]
    # ties: 64 key values per tile, so (tile, key) pairs repeat -- at least 5 % of the instances share theirs
    assert np.unique(x["e"]["keys_sorted"]).size <= 0.95 * x["e"]["V"]
    if not x["claims"]["empty_first_and_last"]:
        assert (lens > 0).all()


def _claim_empty_first_and_last(v, x):
    rg = x["e"]["ranges"]
    assert (bool((rg[0] == 0).all() and (rg[-1] == 0).all() and rg.shape[0] > 2)) == v
    if v:
        lens = rg[:, 1].astype(np.int64) - rg[:, 0]
        assert (lens[1:-1] == 0).any() and (lens[1:-1] > 0).sum() >= rg.shape[0] // 2   # and some in between


CHECKERS = {
    "P": lambda v, x: x["keys"].size == v,
    "V": lambda v, x: int(x["visible"].sum()) == v == x["e"]["num_rendered"],
    "far": lambda v, x: x["e"]["far"] == v,
    "span": lambda v, x: x["e"]["span"] == v,
    "min_key": lambda v, x: x["e"]["min_key"] == v,
    "max_key": lambda v, x: x["e"]["max_key"] == v,
    "both_cull_rules": lambda v, x: v and {1, 2} <= set(np.unique(x["cull"]).tolist()),
    "culled_rule": lambda v, x: set(np.unique(x["cull"]).tolist()) == {0, v},
    "dead_chunks": _claim_dead_chunks,
    "only_visible_id": lambda v, x: np.nonzero(x["visible"])[0].tolist() == [v] and v // C == (x["P"] - 1) // C
    and x["P"] % C != 0,
    "distinct_keys": lambda v, x: np.unique(x["keys"][x["visible"]]).size == v,
    "equal_keys_straddle_every_seam": _claim_straddle,
    "aligned_runs": _claim_runs,
    "only_digit": _claim_only_digit,
    "digit_values": lambda v, x: "only_digit" in x["claims"],
    "max_minus_min_below_2p27": lambda v, x: v and x["e"]["max_key"] - x["e"]["min_key"] < dt.NEAR_SPAN <= x["e"]["span"],
    "far_if_culled_counted": _claim_far_if_culled_counted,
    "rows": lambda v, x: -(-x["P"] // C) == v,
    "fat": lambda v, x: (-(-x["P"] // C) <= dt.DS_MAX_CHUNKS) == v,
    "p_mod_rs_chunk": lambda v, x: x["P"] % dt.RS_CHUNK == v and x["P"] > dt.DS_MAX_CHUNKS * C + 1,
    "tiles": _claim_tiles,
    "empty_first_and_last": _claim_empty_first_and_last,
    "wider_than_255": lambda v, x: (x["gx"] > 255) == v,
    "partition_chunks": lambda v, x: -(-x["e"]["num_rendered"] // dt.RS_CHUNK) == v,
}


@pytest.mark.parametrize("name", list(dt.CASES))
def test_case_is_its_key_set_and_has_the_property_it_claims(name):
    keys, tile, gx, gy, cull, sc, cam, visible = dt.build(name)
    e = dt.conditions(sc, cam, keys, tile, visible)
    claims = dt.CASES[name].claims
    x = dict(keys=keys, tile=tile, gx=gx, gy=gy, cull=cull, visible=visible, e=e, P=keys.size, claims=claims)
    assert claims
    for k, v in claims.items():
        assert k in CHECKERS, "claim without a checker: " + k
        assert CHECKERS[k](v, x) is not False, (name, k, v)
    # the truth accepts itself
    dt.compare(dt.as_frame(e, keys, visible), e, keys, visible)


def test_the_case_table_covers_what_it_must():
    P = {k: c.claims["P"] for k, c in dt.CASES.items()}
    assert {P[k] for k in dt.CASES if k.startswith("p_")} == {1, C - 1, C, C + 1, 2 * C, 2 * C + 1}
    assert {dt.CASES[k].claims["V"] for k in dt.CASES if k.startswith("v_")} == {2 * C - 1, 2 * C, 2 * C + 1}
    assert P["rows_128"] == 128 * C and P["rows_129"] == 128 * C + 1
    assert P["fat_512_chunks"] == 512 * C and P["classic_512_chunks_plus_1"] == 512 * C + 1
    seam = 512 * C + 1 + dt.RS_CHUNK * dt.CLASSIC_K
    assert [P["classic_seam_" + t] for t in ("minus_1", "exact", "plus_1")] == [seam - 1, seam, seam + 1]
    assert (seam - 1) % dt.RS_CHUNK == 0
    assert sorted(gx * gy for gx, gy in dt.GRIDS) == [1, 2, 128, 129, 256, 257]
    # 257 x 1 is the only grid wider than 255 tiles: the route without the rectangle payload
    assert [g for g in dt.GRIDS if g[0] > 255 or g[1] > 255] == [(257, 1)]
    for gx, gy in dt.GRIDS:
        for R in (dt.RS_CHUNK - 1, dt.RS_CHUNK, dt.RS_CHUNK + 1):
            assert "tiles_%dx%d_r%d" % (gx, gy, R) in dt.PARTITION
    assert dt.PARTITION_BIG == 1024 * dt.RS_CHUNK + 1
    assert all(k in dt.CASES for k in dt.COMPOSED + dt.RANGE)
    assert {dt.CASES[k].claims["far"] for k in dt.RANGE} == {True, False}


# ----------------------------------------------------------------------------------------------------------------
# planted errors: the comparison rejects what a seam bug produces
# ----------------------------------------------------------------------------------------------------------------
def _built(name):
    keys, tile, gx, gy, cull, sc, cam, visible = dt.build(name)
    return keys, tile, gx, gy, cull, visible, dt.expected(keys, tile, visible, gx, gy)


def test_planted_swap_of_equal_keys_across_a_chunk_seam_is_rejected():
    keys, tile, gx, gy, cull, visible, e = _built("equal_keys")
    for s in range(C, keys.size, C):
        t = int(tile[s])
        i = int(np.nonzero(tile[:s] == t)[0][-1])          # the last id of this tile before the seam, the first behind
        pl = e["point_list"].astype(np.int64)
        a, b = int(np.nonzero(pl == i)[0][0]), int(np.nonzero(pl == s)[0][0])
        assert b == a + 1 and keys[i] == keys[s]
        pl[a], pl[b] = pl[b], pl[a]
        wrong = dt.with_point_list(e, keys, tile, visible, pl)
        np.testing.assert_array_equal(wrong["keys_sorted"], e["keys_sorted"])     # only the ids show it
        with pytest.raises(AssertionError, match="point_list"):
            dt.compare(wrong, e, keys, visible)


def test_planted_drop_of_the_last_visible_entry_is_rejected():
    name = "v_%d_of_%d" % (2 * C, 3 * C + 77)
    keys, tile, gx, gy, cull, visible, e = _built(name)
    wrong = dt.with_point_list(e, keys, tile, visible, e["point_list"][:-1])
    with pytest.raises(AssertionError):
        dt.compare(wrong, e, keys, visible)
    # the count right, the last entry overwritten by its neighbour (a rank one too low at the end of the last chunk)
    pl = e["point_list"].copy()
    pl[-1] = pl[-2]
    with pytest.raises(AssertionError, match="keys_sorted|point_list"):
        dt.compare(dt.with_point_list(e, keys, tile, visible, pl), e, keys, visible)


@pytest.mark.parametrize("rule", [dt.CULL_NEAR_PLANE, dt.CULL_SIDEWAYS])
def test_planted_culled_id_kept_is_rejected(rule):
    name = "v_%d_of_%d" % (2 * C, 3 * C + 77)
    keys, tile, gx, gy, cull, visible, e = _built(name)
    kept = visible.copy()
    kept[int(np.nonzero(cull == rule)[0][0])] = True
    wrong = dt.with_point_list(e, keys, tile, visible, dt.expected(keys, tile, kept, gx, gy)["point_list"])
    with pytest.raises(AssertionError):
        dt.compare(wrong, e, keys, visible)


@pytest.mark.parametrize("name", [k for k in dt.RANGE + ("digit_pass3",) if dt.CASES[k].claims["far"]])
def test_planted_27_bit_order_is_rejected_in_the_far_cases(name):
    keys, tile, gx, gy, cull, visible, e = _built(name)
    assert e["far"]
    pl = dt.truncated_order(keys, tile, visible, e)
    assert (pl != e["point_list"]).any()
    with pytest.raises(AssertionError, match="keys_sorted"):
        dt.compare(dt.with_point_list(e, keys, tile, visible, pl), e, keys, visible)


@pytest.mark.parametrize("name", [k for k in dt.RANGE if not dt.CASES[k].claims["far"]])
def test_27_bit_order_is_the_order_in_the_near_cases(name):
    keys, tile, gx, gy, cull, visible, e = _built(name)
    np.testing.assert_array_equal(dt.truncated_order(keys, tile, visible, e), e["point_list"])
