"""Scenes built FROM a list of depth keys, and the exact binning they must give: the depth sort (csrc/sort.hip) and the
tile partition (sort_binning / the hierarchical route's coarse partition) at their chunk and range edges.

hz.trajectory_camera(0, W, H) has an identity view matrix, so a Gaussian's depth key is the bit pattern of its z.  A
scene is therefore made from uint32 keys: z = key.view(float32), pixel centre uniform in [4, 12) of a chosen tile,
isotropic scale 0.3 z / fx (radius 2 px: the rectangle never leaves the tile, tiles_touched == 1, R == V), identity
quaternion, opacity 0.5, SH degree 0.  The truth is then three lines of numpy -- the visible ids in (tile, key, id)
order -- which `conditions` confirms against the CPU oracle before any GPU test uses it.  Everything compared is an
integer: there is no tolerance anywhere in this file.

  key_scene     (Scene, CameraTensors, visible) from keys, tiles and a per-Gaussian cull rule.
  expected      point_list / keys_sorted / ranges / num_rendered / key_base / span / far in numpy alone.
  conditions    what makes a case mean something, from oracle.forward(render=False); asserted on the host and again
                by every GPU test on its own inputs.
  compare       exact equality of a decoded frame with `expected`; the GPU tests call it, the host test shows that
                it rejects planted mistakes.
  CASES         name -> Case(build, claims): the inputs that sit ON a seam, and the property each one claims as data
                (tests/test_depth_sort_host.py asserts every claim, so a case that stops exercising its seam fails
                there instead of passing silently on the GPU).

Nothing here runs on the GPU.
"""
import zlib
from typing import Callable, NamedTuple

import numpy as np
import torch

from gaussianrpg_amd import harness as hz

# csrc/common.h (asserted against its text by tests/test_depth_sort_host.py)
DS_CHUNK = 8192          # keys per workgroup of the fat depth sort
DS_BITS = 9              # bits per fat pass
DS_MAX_CHUNKS = 512      # beyond: the classic histogram / digit-scan / scatter passes
RS_CHUNK = 2048          # keys per workgroup of the classic radix passes (tile partition, classic depth sort)
KEY_ALIGN = 1 << 18      # key_base = smallest visible key rounded down to this (sort.hip publish_frame_counts)
CULLED_KEY = 0xFFFFFFFF

C = DS_CHUNK
NEAR_SPAN = 1 << (3 * DS_BITS)      # far  <=>  (max_key - key_base) >> 27 != 0

CULL_NONE, CULL_NEAR_PLANE, CULL_SIDEWAYS = 0, 1, 2


def bits(z):
    return int(np.float32(z).view(np.uint32))


BASE = bits(2.0) & ~(KEY_ALIGN - 1)
KEY_021 = bits(0.21)                # nearest depth of the deep cases (the near plane culls z <= 0.2)
KEY_2P60 = bits(2.0 ** 60)          # farthest


def key_scene(keys, tile, gx, gy, cull=None, seed=0):
    """(Scene, CameraTensors, visible bool[P]) under hz.trajectory_camera(0, 16 gx, 16 gy).
    cull[i]: 0 visible | 1 behind the near plane (z = 0.1: its key is never seen) | 2 outside the frustum sideways
    (pixel x = -5000: keeps its z, a valid depth whose key must NOT reach the frame's min / max)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    tile = np.asarray(tile, dtype=np.int64)
    P = keys.shape[0]
    cull = np.zeros(P, np.uint8) if cull is None else np.asarray(cull, dtype=np.uint8)
    assert tile.shape == (P,) and cull.shape == (P,)
    assert P == 0 or (0 <= tile.min() and tile.max() < gx * gy)
    W, H = 16 * int(gx), 16 * int(gy)
    cam = hz.trajectory_camera(0, W=W, H=H)
    fx = W / (2.0 * cam.tanfovx)
    fy = H / (2.0 * cam.tanfovy)
    r = np.random.RandomState(seed)
    u = 4.0 + 8.0 * r.rand(P, 2)
    px = 16.0 * (tile % gx) + u[:, 0]
    py = 16.0 * (tile // gx) + u[:, 1]
    z = keys.view(np.float32).astype(np.float64)
    z = np.where(cull == CULL_NEAR_PLANE, 0.1, z)
    px = np.where(cull == CULL_SIDEWAYS, -5000.0, px)
    # ndc2Pix: pixel = ((ndc + 1) S - 1) / 2 with ndc = 2 f x / (S z)  ->  x = (pixel + 0.5 - S / 2) z / f
    means = np.stack([(px + 0.5 - 0.5 * W) * z / fx, (py + 0.5 - 0.5 * H) * z / fy, z], 1)
    scales = np.repeat((0.3 * z / fx)[:, None], 3, 1)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))   # noqa: E731
    quat = np.zeros((P, 4), np.float32)
    quat[:, 0] = 1.0
    shs = -1.0 + 3.0 * r.rand(P, 1, 3)
    sc = hz.Scene(f(means), torch.full((P, 1), 0.5), f(scales), torch.from_numpy(quat), f(shs), 0)
    return sc, cam, cull == CULL_NONE


def expected(keys, tile, visible, gx, gy):
    """The truth in numpy alone: the visible ids by (tile, key, id)."""
    keys = np.asarray(keys, dtype=np.uint32)
    tile = np.asarray(tile, dtype=np.int64)
    ids = np.nonzero(np.asarray(visible, bool))[0]
    order = ids[np.lexsort((ids, keys[ids], tile[ids]))]
    T = int(gx) * int(gy)
    ts = tile[order]
    lo, hi = np.searchsorted(ts, np.arange(T), "left"), np.searchsorted(ts, np.arange(T), "right")
    ranges = np.stack([lo, hi], 1).astype(np.uint32)
    ranges[lo == hi] = 0                                         # an empty tile keeps the cleared (0, 0)
    out = dict(point_list=order.astype(np.uint32),
               keys_sorted=(ts.astype(np.uint64) << np.uint64(32)) | keys[order].astype(np.uint64),
               ranges=ranges, num_rendered=int(ids.size), V=int(ids.size))
    if ids.size:
        kmin, kmax = int(keys[ids].min()), int(keys[ids].max())
        out.update(min_key=kmin, max_key=kmax, key_base=kmin & ~(KEY_ALIGN - 1))
        out["span"] = kmax - out["key_base"]
        out["far"] = (out["span"] >> (3 * DS_BITS)) != 0
    else:                                                        # nothing visible: any base will do, never far
        out.update(min_key=None, max_key=None, key_base=0, span=0, far=False)
    return out


def oracle_binning(sc, cam):
    import oracle
    from helpers import oracle_kwargs
    return oracle.forward(sc.means3D, sc.opacity, shs=sc.shs, scales=sc.scales, rotations=sc.rotations, render=False,
                          **oracle_kwargs(cam, sc.sh_degree))


def conditions(sc, cam, keys, tile, visible):
    """Asserts that the scene IS the crafted key set (from the CPU oracle's preprocess and binning) and returns
    `expected`: visibility as intended, key bits exact, one tile per visible Gaussian (so R == V), and the oracle's
    own point list / ranges / count equal to the numpy truth."""
    keys = np.asarray(keys, dtype=np.uint32)
    visible = np.asarray(visible, bool)
    o = oracle_binning(sc, cam)
    gx, gy = o["grid"]
    e = expected(keys, tile, visible, gx, gy)
    np.testing.assert_array_equal(o["radii"] > 0, visible)
    np.testing.assert_array_equal(o["depths"].view(np.uint32)[visible], keys[visible])
    np.testing.assert_array_equal(o["tiles_touched"], visible.astype(np.uint32))
    assert o["num_rendered"] == e["num_rendered"] == int(visible.sum())
    np.testing.assert_array_equal(o["point_list"], e["point_list"])
    np.testing.assert_array_equal(o["keys_sorted"], e["keys_sorted"])
    np.testing.assert_array_equal(o["ranges"], e["ranges"])
    return e


def compare(got, e, keys, visible):
    """Exact equality of a decoded frame (`got`: num_rendered, radii, depths, tiles_touched, keys_sorted, point_list,
    ranges as numpy arrays) with the truth `e`."""
    keys = np.asarray(keys, dtype=np.uint32)
    visible = np.asarray(visible, bool)
    assert int(got["num_rendered"]) == e["num_rendered"], (int(got["num_rendered"]), e["num_rendered"])
    np.testing.assert_array_equal(np.asarray(got["radii"]) > 0, visible, err_msg="radii > 0")
    np.testing.assert_array_equal(np.ascontiguousarray(got["depths"]).view(np.uint32)[visible], keys[visible],
                                  err_msg="depth keys")
    np.testing.assert_array_equal(np.ascontiguousarray(got["tiles_touched"]).view(np.uint32),
                                  visible.astype(np.uint32), err_msg="tiles_touched")
    np.testing.assert_array_equal(np.ascontiguousarray(got["keys_sorted"]).view(np.uint64), e["keys_sorted"],
                                  err_msg="keys_sorted")
    np.testing.assert_array_equal(np.ascontiguousarray(got["point_list"]).view(np.uint32), e["point_list"],
                                  err_msg="point_list")
    np.testing.assert_array_equal(np.ascontiguousarray(got["ranges"]).view(np.uint32).reshape(-1, 2), e["ranges"],
                                  err_msg="ranges")


def as_frame(e, keys, visible):
    """The truth in the shape `compare` takes a decoded frame in (the host test plants its mistakes into this)."""
    keys = np.asarray(keys, dtype=np.uint32)
    visible = np.asarray(visible, bool)
    return dict(num_rendered=e["num_rendered"], radii=np.where(visible, 2, 0).astype(np.int32),
                depths=np.where(visible, keys, 0).astype(np.uint32).view(np.float32),
                tiles_touched=visible.astype(np.int32), keys_sorted=e["keys_sorted"].copy(),
                point_list=e["point_list"].copy(), ranges=e["ranges"].copy())


def with_point_list(e, keys, tile, visible, point_list):
    """A decoded frame whose point list is `point_list` (keys_sorted and ranges follow it, as they would on the
    device: the key of an instance is read from the Gaussian it names)."""
    keys = np.asarray(keys, dtype=np.uint32)
    tile = np.asarray(tile, dtype=np.int64)
    fr = as_frame(e, keys, visible)
    pl = np.asarray(point_list, dtype=np.int64)
    fr["point_list"] = pl.astype(np.uint32)
    fr["keys_sorted"] = (tile[pl].astype(np.uint64) << np.uint64(32)) | keys[pl].astype(np.uint64)
    fr["num_rendered"] = int(pl.size)
    return fr


def truncated_order(keys, tile, visible, e):
    """The point list of a sort that orders (key - key_base) & (2^27 - 1): three passes on a frame that needs four."""
    keys = np.asarray(keys, dtype=np.uint32)
    tile = np.asarray(tile, dtype=np.int64)
    ids = np.nonzero(np.asarray(visible, bool))[0]
    k27 = (keys[ids].astype(np.int64) - e["key_base"]) & (NEAR_SPAN - 1)
    return ids[np.lexsort((ids, k27, tile[ids]))]


def digits(keys, key_base, p):
    """Digit of pass p of the fat sort: bits [9p, 9p + 9) of key - key_base (p = 3: the remaining bits [27, 32))."""
    d = (np.asarray(keys, dtype=np.int64) - int(key_base)) >> (DS_BITS * p)
    return d if p == 3 else d & ((1 << DS_BITS) - 1)


# ------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    build: Callable        # () -> (keys uint32[P], tile int64[P], gx, gy, cull uint8[P])
    claims: dict           # the property the case stands for, as data (test_depth_sort_host.py: check_claims)


CASES = {}


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def _random_tiles(r, P, T, empty=()):
    allowed = np.setdiff1d(np.arange(T), np.asarray(empty, dtype=np.int64))
    return allowed[r.randint(0, allowed.size, P)]


def _cull_exactly(r, P, n_culled):
    """n_culled random ids culled, rules 1 and 2 in turn."""
    cull = np.zeros(P, np.uint8)
    ids = r.permutation(P)[:n_culled]
    cull[ids[0::2]] = CULL_NEAR_PLANE
    cull[ids[1::2]] = CULL_SIDEWAYS
    return cull


def _near_keys(r, P, span=NEAR_SPAN):
    return (BASE + r.randint(0, span, P).astype(np.int64)).astype(np.uint32)


def _deep_keys(r, P):
    return r.randint(KEY_021, KEY_2P60 + 1, P).astype(np.uint32)


def _case(name, claims):
    def deco(fn):
        CASES[name] = Case(lambda: fn(_rng(name)), dict(claims))
        return fn
    return deco


# --- chunk seams of the fat sort: P and V -------------------------------------------------------------------------
def _all_visible(P):
    def build(r):
        return _near_keys(r, P), _random_tiles(r, P, 2), 2, 1, np.zeros(P, np.uint8)
    return build


for _P in (1, C - 1, C, C + 1, 2 * C, 2 * C + 1):
    _case("p_%d" % _P, dict(P=_P, V=_P, far=False))(_all_visible(_P))


def _v_on_seam(V):
    P = 3 * C + 77

    def build(r):
        return _near_keys(r, P), _random_tiles(r, P, 2), 2, 1, _cull_exactly(r, P, P - V)
    return build


for _V in (2 * C - 1, 2 * C, 2 * C + 1):
    _case("v_%d_of_%d" % (_V, 3 * C + 77), dict(P=3 * C + 77, V=_V, far=False, both_cull_rules=True))(_v_on_seam(_V))


@_case("dead_chunk", dict(P=3 * C, V=2 * C, dead_chunks=(1,), both_cull_rules=True))
def _dead_chunk(r):
    P = 3 * C
    cull = np.zeros(P, np.uint8)
    cull[C:2 * C:2] = CULL_NEAR_PLANE
    cull[C + 1:2 * C:2] = CULL_SIDEWAYS
    return _near_keys(r, P), _random_tiles(r, P, 2), 2, 1, cull


@_case("all_dead_3_chunks", dict(P=2 * C + 5, V=0, dead_chunks=(0, 1, 2), both_cull_rules=True))
def _all_dead(r):
    P = 2 * C + 5
    cull = np.full(P, CULL_NEAR_PLANE, np.uint8)
    cull[1::2] = CULL_SIDEWAYS
    return _near_keys(r, P), _random_tiles(r, P, 2), 2, 1, cull


@_case("one_visible_in_last_chunk", dict(P=2 * C + 5, V=1, dead_chunks=(0, 1), only_visible_id=2 * C + 3,
                                         both_cull_rules=True))
def _one_visible(r):
    P = 2 * C + 5
    cull = np.full(P, CULL_NEAR_PLANE, np.uint8)
    cull[1::2] = CULL_SIDEWAYS
    cull[2 * C + 3] = CULL_NONE
    return _near_keys(r, P), _random_tiles(r, P, 2), 2, 1, cull


# --- stability across (chunk, wave, round, lane) ------------------------------------------------------------------
@_case("equal_keys", dict(P=2 * C + 513, V=2 * C + 513, distinct_keys=1, equal_keys_straddle_every_seam=True))
def _equal_keys(r):
    P = 2 * C + 513
    return np.full(P, BASE + 0x2345678, np.uint32), _random_tiles(r, P, 2), 2, 1, np.zeros(P, np.uint8)


def _runs(run):
    # aligned runs: every block of `run` consecutive ids -- a wave round (64), a wave's share (512), a chunk (8192) of
    # depth_scatter_kernel -- holds ONE key value, and the larger value comes first, so every block has to move
    P = 3 * C + 513

    def build(r):
        hi, lo = BASE + 0x5A5A5A5, BASE + 0x25A5A5A
        keys = np.where((np.arange(P) // run) % 2 == 0, hi, lo).astype(np.uint32)
        return keys, _random_tiles(r, P, 2), 2, 1, np.zeros(P, np.uint8)
    return build


for _run in (64, 512, C):
    _case("runs_%d" % _run, dict(P=3 * C + 513, V=3 * C + 513, distinct_keys=2, aligned_runs=_run))(_runs(_run))

# The digit values bits [27, 32) of key - key_base can take at all: positive floats in [0.21, 2^60] span
# bits(2^60) - (bits(0.21) & ~0x3FFFF) = 0x1F2C0000 key values, so the fourth pass sees the digits 0, 1, 2, 3 and no
# others (test_depth_sort_host.py: test_the_fourth_pass_digits_floats_reach); the case populates all four.
PASS3_DIGITS = (0, 1, 2, 3)


def _one_digit(p):
    P = C + 100
    values = np.asarray(PASS3_DIGITS) if p == 3 else np.arange(1 << DS_BITS)
    origin = KEY_021 if p == 3 else BASE

    def build(r):
        d = np.concatenate([values, values[r.randint(0, values.size, P - values.size)]])
        keys = (origin + (d[r.permutation(P)].astype(np.int64) << (DS_BITS * p))).astype(np.uint32)
        return keys, _random_tiles(r, P, 2), 2, 1, np.zeros(P, np.uint8)
    return build


for _p in range(4):
    _case("digit_pass%d" % _p, dict(P=C + 100, V=C + 100, only_digit=_p, far=_p == 3,
                                    digit_values=PASS3_DIGITS if _p == 3 else tuple(range(1 << DS_BITS))))(_one_digit(_p))


# --- the range decision: key_base = min & ~0x3FFFF, far <=> (max - key_base) >> 27 != 0 ---------------------------
def _range_case(kmin, kmax, culled_key=None, rule=CULL_NONE, P=3000, n_culled=50):
    def build(r):
        keys = r.randint(kmin, kmax + 1, P).astype(np.uint32)
        ids = r.permutation(P)
        keys[ids[0]], keys[ids[1]] = kmin, kmax
        cull = np.zeros(P, np.uint8)
        if culled_key is not None:
            keys[ids[2:2 + n_culled]] = culled_key
            cull[ids[2:2 + n_culled]] = rule
        return keys, _random_tiles(r, P, 2), 2, 1, cull
    return build


_LOW = KEY_ALIGN - 1     # 0x3FFFF: the bits key_base drops
_case("span_2p27_minus_1", dict(P=3000, V=3000, min_key=BASE, span=NEAR_SPAN - 1, far=False))(
    _range_case(BASE, BASE + NEAR_SPAN - 1))
_case("span_2p27", dict(P=3000, V=3000, min_key=BASE, span=NEAR_SPAN, far=True))(
    _range_case(BASE, BASE + NEAR_SPAN))
_case("min_low_bits_far", dict(P=3000, V=3000, min_key=BASE + _LOW, span=NEAR_SPAN, far=True,
                               max_minus_min_below_2p27=True))(
    _range_case(BASE + _LOW, BASE + NEAR_SPAN))
_case("min_low_bits_near", dict(P=3000, V=3000, min_key=BASE + _LOW, span=NEAR_SPAN - 1, far=False))(
    _range_case(BASE + _LOW, BASE + NEAR_SPAN - 1))
_case("culled_below_near_plane", dict(P=3000, V=2950, min_key=BASE + _LOW, span=NEAR_SPAN - 1, far=False,
                                      culled_rule=CULL_NEAR_PLANE, far_if_culled_counted=True))(
    _range_case(BASE + _LOW, BASE + NEAR_SPAN - 1, bits(0.25), CULL_NEAR_PLANE))
_case("culled_below_sideways", dict(P=3000, V=2950, min_key=BASE + _LOW, span=NEAR_SPAN - 1, far=False,
                                    culled_rule=CULL_SIDEWAYS, far_if_culled_counted=True))(
    _range_case(BASE + _LOW, BASE + NEAR_SPAN - 1, bits(0.25), CULL_SIDEWAYS))
_case("culled_above_sideways", dict(P=3000, V=2950, min_key=BASE + _LOW, span=NEAR_SPAN - 1, far=False,
                                    culled_rule=CULL_SIDEWAYS, far_if_culled_counted=True))(
    _range_case(BASE + _LOW, BASE + NEAR_SPAN - 1, bits(2.0 ** 40), CULL_SIDEWAYS))
_case("deep_range", dict(P=3000, V=3000, min_key=KEY_021, max_key=KEY_2P60, far=True))(
    _range_case(KEY_021, KEY_2P60))


# --- the table sweep: wave w owns rows w, w + 16, ...; eight per round, so the second round starts at 129 rows ------
def _sweep(P):
    def build(r):
        keys = _near_keys(r, P, 1 << 20)                      # ~1 key value per Gaussian: ties are frequent
        return keys, _random_tiles(r, P, 16), 4, 4, _cull_exactly(r, P, P // 10)
    return build


_case("rows_128", dict(P=128 * C, V=128 * C - 128 * C // 10, rows=128, far=False, both_cull_rules=True))(_sweep(128 * C))
_case("rows_129", dict(P=128 * C + 1, V=128 * C + 1 - (128 * C + 1) // 10, rows=129, far=False,
                       both_cull_rules=True))(_sweep(128 * C + 1))


# --- the switch to the classic passes: P <= 512 C fat, beyond classic (culled keys sort last, V stays P) ----------
def _switch(P):
    def build(r):
        return _deep_keys(r, P), _random_tiles(r, P, 16), 4, 4, _cull_exactly(r, P, P // 5)
    return build


_FAT_MAX = DS_MAX_CHUNKS * C
_case("fat_512_chunks", dict(P=_FAT_MAX, V=_FAT_MAX - _FAT_MAX // 5, rows=512, fat=True, both_cull_rules=True))(
    _switch(_FAT_MAX))
_case("classic_512_chunks_plus_1", dict(P=_FAT_MAX + 1, V=_FAT_MAX + 1 - (_FAT_MAX + 1) // 5, fat=False,
                                        both_cull_rules=True))(_switch(_FAT_MAX + 1))
# a chunk seam of the classic passes (2048 keys per workgroup), one chunk beyond the switch:
# P = 512 C + 1 + 2048 k + {-1, 0, 1} with k = 1, i.e. 2049 * 2048 + {0, 1, 2}  (512 C + 1 itself is 2048 * 2048 + 1)
CLASSIC_K = 1
for _d, _tag in ((-1, "minus_1"), (0, "exact"), (1, "plus_1")):
    _P = _FAT_MAX + 1 + RS_CHUNK * CLASSIC_K + _d
    _case("classic_seam_" + _tag, dict(P=_P, V=_P - _P // 5, fat=False, p_mod_rs_chunk=1 + _d,
                                        both_cull_rules=True))(_switch(_P))


# --- the tile partition: bits_for(T) bits over R = V instances ----------------------------------------------------
GRIDS = ((1, 1), (2, 1), (16, 8), (43, 3), (16, 16), (257, 1))      # T = 1, 2, 128, 129, 256, 257


def _partition(gx, gy, R):
    T = gx * gy

    def build(r):
        # tile 0 and the last tile are left empty, and every tenth in between (grids of one or two tiles use them all)
        empty = () if T <= 2 else tuple(sorted({0, T - 1} | set(range(7, T - 1, 10))))
        keys = (BASE + r.randint(0, 64, R)).astype(np.uint32)      # 64 key values: many ties in every tile
        return keys, _random_tiles(r, R, T, empty), gx, gy, np.zeros(R, np.uint8)
    return build


for _gx, _gy in GRIDS:
    for _R in (RS_CHUNK - 1, RS_CHUNK, RS_CHUNK + 1):
        _T = _gx * _gy
        _case("tiles_%dx%d_r%d" % (_gx, _gy, _R),
              dict(P=_R, V=_R, tiles=_T, far=False, empty_first_and_last=_T > 2, wider_than_255=_gx > 255))(
            _partition(_gx, _gy, _R))
# the second round of radix_digit_scan_kernel's loop over chunks starts at 1025 chunks
PARTITION_BIG = 1024 * RS_CHUNK + 1
_case("tiles_16x16_r%d" % PARTITION_BIG,
      dict(P=PARTITION_BIG, V=PARTITION_BIG, tiles=256, far=False, empty_first_and_last=True, wider_than_255=False,
           partition_chunks=1025))(_partition(16, 16, PARTITION_BIG))

SEAMS = tuple(k for k in CASES if k.startswith(("p_", "v_"))) + ("dead_chunk", "all_dead_3_chunks",
                                                                 "one_visible_in_last_chunk")
STABILITY = ("equal_keys",) + tuple(k for k in CASES if k.startswith(("runs_", "digit_pass")))
RANGE = ("span_2p27_minus_1", "span_2p27", "min_low_bits_far", "min_low_bits_near", "culled_below_near_plane",
         "culled_below_sideways", "culled_above_sideways", "deep_range")
PARTITION = tuple(k for k in CASES if k.startswith("tiles_") and CASES[k].claims["P"] <= RS_CHUNK + 1)
SMALL = SEAMS + STABILITY + RANGE + PARTITION
# a million Gaussians and more: the default route and sort_binning only
BIG = ("rows_128", "rows_129", "tiles_16x16_r%d" % PARTITION_BIG, "fat_512_chunks", "classic_512_chunks_plus_1",
       "classic_seam_minus_1", "classic_seam_exact", "classic_seam_plus_1")
assert set(SMALL) | set(BIG) == set(CASES) and not set(SMALL) & set(BIG)
COMPOSED = ("v_%d_of_%d" % (2 * C, 3 * C + 77), "span_2p27")


def build(name, seed=0):
    """(keys, tile, gx, gy, cull, Scene, CameraTensors, visible) of a case."""
    keys, tile, gx, gy, cull = CASES[name].build()
    sc, cam, visible = key_scene(keys, tile, gx, gy, cull, seed=seed)
    return keys, tile, gx, gy, cull, sc, cam, visible
