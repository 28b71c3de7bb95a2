"""The pictures and unit lists of the TZ search tests, on the host: tests/test_tz_oracle.py proves on the CPU that they reach
every branch of the walk, tests/test_gpu_tz_search.py runs them on the device.  A 192 x 128 picture with margin 80, as
tests/test_gpu_me.py; no GPU and no library needed (the box and the start points come from tests/me_oracle.py).

scenes(B) -> list of Scene(name, refs, org, units, tz, lam): refs = luma planes WITH margins, org = the original luma plane,
units / tz = arrays with the fields of hmx_me_unit / hmx_tz_unit (plain numpy dtypes equal to capi's)."""
import collections

import numpy as np

import me_oracle as mo

W, H, M = 192, 128, 80
ME_UNIT_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("w", "u1"), ("h", "u1"), ("ref", "u1"), ("sub_shift", "u1"), ("pred_x", "<i2"),
                          ("pred_y", "<i2"), ("left", "<i2"), ("top", "<i2"), ("right", "<i2"), ("bottom", "<i2")])
TZ_UNIT_DTYPE = np.dtype([("start_x", "<i2"), ("start_y", "<i2"), ("range", "<u2"), ("reserved", "<u2")])
Scene = collections.namedtuple("Scene", "name refs org units tz lam")


def textured_host(B):
    """What test_gpu_me.make_textured uploads (the GPU test asserts the equality): true displacement (-2, 3) on reference 0."""
    rng = np.random.default_rng(800 + B)
    refs = []
    for k in range(2):
        yy, xx = np.mgrid[0:H + 2 * M, 0:W + 2 * M]
        base = (np.sin(xx / (5.0 + k)) + np.cos(yy / (7.0 - k))) * (1 << (B - 3)) + (1 << (B - 1))
        refs.append(np.clip(base + rng.integers(-(1 << (B - 4)), 1 << (B - 4), base.shape), 0, (1 << B) - 1).astype(np.int16))
    org = np.clip(refs[0][M + 3:M + 3 + H, M - 2:M - 2 + W].astype(np.int32) + rng.integers(-6, 7, (H, W)), 0, (1 << B) - 1).astype(np.int16)
    return refs, org


def _box(a, n):
    """Sums over n x n windows, integer arithmetic."""
    c = np.cumsum(np.cumsum(a, 0), 1)
    c = np.pad(c, ((1, 0), (1, 0)))
    return c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]


TRUE_MV = (7, -5)


def smooth_host(B):
    """Low-passed noise (two 9 x 9 box sums, stretched), all in integers: the SAD falls towards the true displacement without
    periodic minima.  The original is reference 0 displaced by TRUE_MV exactly; reference 1 holds the original at displacement
    (0, 0) and reference 0's samples elsewhere, so a unit on reference 1 finds the zero vector best."""
    rng = np.random.default_rng(1700 + B)
    n = rng.integers(0, 1 << B, (H + 2 * M + 16, W + 2 * M + 16)).astype(np.int64)
    s = _box(_box(n, 9), 9)  # mean 81 * 81 * 2^(B-1)
    mid = 81 * 81 * (((1 << B) - 1) / 2.0)
    ref0 = np.clip((s - int(mid)) * 6 // (81 * 81) + (1 << (B - 1)), 0, (1 << B) - 1).astype(np.int16)
    assert ref0.shape == (H + 2 * M, W + 2 * M)
    org = ref0[M + TRUE_MV[1]:M + TRUE_MV[1] + H, M + TRUE_MV[0]:M + TRUE_MV[0] + W].copy()
    ref1 = ref0.copy()
    ref1[M:M + H, M:M + W] = org
    return [ref0, ref1], org


def unit(x, y, w, h, ref, s, px, py, box):
    u = np.zeros(1, ME_UNIT_DTYPE)
    u[0] = (x, y, w, h, ref, s, px, py) + tuple(box)
    return u


def boxed(x, y, w, h, ref, s, px, py, rng_):
    """(unit, tz) as xMotionEstimation makes them: xSetSearchRange around the predictor, start = clipMv(predictor) >> 2."""
    u = unit(x, y, w, h, ref, s, px, py, mo.set_search_range(px, py, rng_, x, y, W, H, 64))
    cx, cy = mo.clip_mv(px, py, x, y, W, H, 64)
    z = np.zeros(1, TZ_UNIT_DTYPE)
    z[0] = (cx >> 2, cy >> 2, rng_, 0)
    return u, z


def _cat(pairs):
    return np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])


SHAPES = [(8, 4), (4, 8), (12, 16), (16, 4), (24, 32), (64, 48), (64, 64), (4, 4), (8, 8), (16, 12), (32, 24), (48, 64), (32, 32), (16, 16),
          (48, 16), (16, 64), (24, 8), (12, 48)]


def textured_units(B):
    rng = np.random.default_rng(1720 + B)
    pairs = []
    for k, (w, h) in enumerate(SHAPES * 2):
        x, y = int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4
        s = int(h > 8 and k % 2 == 0)
        far = 120 if k % 3 == 0 else 40
        pairs.append(boxed(x, y, w, h, k % 2, s, int(rng.integers(-far, far + 1)), int(rng.integers(-far, far + 1)), (64, 64, 16, 5)[k % 4]))
    for (x, y) in ((0, 0), (W - 16, 0), (0, H - 16), (W - 16, H - 16)):  # picture corners: xSetSearchRange cuts the box
        px, py = (-300 if x == 0 else 300), (-300 if y == 0 else 300)
        pairs.append(boxed(x, y, 16, 16, (x + y) // 16 % 2, 1, px, py, 64))
        pairs.append(boxed(x, y, 16, 16, 0, 0, px // 30, py // 30, 64))
    return _cat(pairs)


NEIGHBOURS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))


def smooth_units(B):
    tx, ty = TRUE_MV
    pairs = []
    # the truth one step from the start point in each of the eight directions: the eight cases of xTZ2PointSearch
    for k, (dx, dy) in enumerate(NEIGHBOURS):
        w, h = ((16, 16), (32, 16), (8, 8), (16, 32))[k % 4]
        pairs.append(boxed(16 + 20 * k, 24 + 8 * (k % 3), w, h, 0, int(h > 8 and k % 2), 4 * (tx - dx), 4 * (ty - dy), 64))
    # starts further off: star refinement over several passes, and starts so far off that the raster search runs
    for k, (dx, dy) in enumerate(((3, 2), (-6, 5), (11, -9), (-20, 13), (30, 22), (-45, -30), (50, -40), (24, 24))):
        w, h = ((32, 32), (16, 8), (64, 64), (8, 16), (24, 24), (48, 32), (12, 12), (4, 4))[k]
        pairs.append(boxed(8 * k + 4, 4 * k, w, h, 0, int(h > 8 and k % 2 == 0), 4 * (tx + dx) + k % 4, 4 * (ty + dy) - k % 3, (64, 32, 64, 8)[k % 4]))
    # reference 1 holds the original at (0, 0): the zero vector wins; the predictor is so far off that (0, 0) lies outside the box
    for k, (px, py, rng_) in enumerate(((40 * 4, 0, 8), (-30 * 4, 25 * 4, 16), (0, -36 * 4, 32), (50 * 4, 50 * 4, 4), (12 * 4, 0, 8))):
        w, h = ((16, 16), (8, 8), (32, 32), (64, 16), (4, 16))[k]
        pairs.append(boxed(64 + 8 * k, 32 + 8 * k, w, h, 1, int(h > 8 and k % 2), px, py, rng_))
    return _cat(pairs)


def const_units():
    """Constant pictures and lambda 0: every cost ties, so the first evaluated point -- the start point -- must win."""
    return _cat([boxed(64, 32, 16, 16, 0, 0, 13, -22, 64), boxed(32, 64, 8, 8, 0, 0, -90, 50, 16), boxed(0, 0, 64, 64, 0, 1, -300, -300, 64),
                 boxed(96, 48, 32, 8, 0, 0, 0, 0, 8)])


_memo = {}


def scenes(B):
    if B not in _memo:
        tr, to = textured_host(B)
        sr, so = smooth_host(B)
        const = [np.full((H + 2 * M, W + 2 * M), (1 << B) - 3, np.int16)]
        corg = np.random.default_rng(1730 + B).integers(0, 1 << B, (H, W)).astype(np.int16)
        _memo[B] = [Scene("textured", tr, to, *textured_units(B), 1234567), Scene("smooth", sr, so, *smooth_units(B), 300000),
                    Scene("constant", const, corg, *const_units(), 0)]
    return _memo[B]
