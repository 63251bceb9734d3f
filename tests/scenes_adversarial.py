"""Hand-built scenes for the places where a BVH walk goes wrong (tests/test_adversarial_walk.py and
tests/test_gpu_adversarial_walk.py).  Small rsd.scenes.Scene objects, every vertex written here.

The frames are odd-sized (65 x 49) with jitter off and no guard band: the centre texel's ray is exactly
the camera axis, and every camera but `grazing`'s looks exactly down -z, so that ray has two zero direction
components (the centre column has d.x = 0, the centre row d.y = 0).

  layers        40 camera-facing quads, each wider than the frustum at its depth, 0.05 apart: every ray has
                >= 40 hits, more than any sorted list holds (K = 4, 8, 16)
  layers_tight  the same quads 3 float ulps apart: pruning among nearly equal keys
  coincident    one quad 9 times over (identical vertices, distinct primitive ids), interleaved in index
                order with a stack of 9 different quads: exact ties in t, and more than kBvhMaxLeaf
                identical centroids (the builder's forced-median split)
  axis_walls    a room on axis planes (flat node boxes) with a partition on x = 0.5 and a shelf on y = 1;
                the camera stands at x = 0.5, y = 1: ray origins in box planes, zero direction components
  grazing       one large floor seen at 0.5 degrees, distant walls: a huge 1 / d on one axis
  slivers       long needles across the view axis at many depths and angles, with zero-area and nearly
                zero-area triangles: overlapping boxes, deep stacks
  far_a_* / far_b_*  layers, coincident, axis_walls and grazing translated by (3000, -500, 7000) and
                (-40000, 0, 25000), camera alike: coarse float spacing in origin x (1 / d)

Every coordinate of coincident and axis_walls is a multiple of 1/256 below 64, so the translations are exact in
float32 there: ties stay ties and the camera stays in its planes."""
from __future__ import annotations

import dataclasses

import numpy as np

from rsd.scenes import FLAG_DOUBLE_SIDED, Scene

W, H = 65, 49
OFFSETS = {"far_a": (3000.0, -500.0, 7000.0), "far_b": (-40000.0, 0.0, 25000.0)}
FAR_BASES = ("layers", "coincident", "axis_walls", "grazing")
LAYER_COUNT, LAYER_Z0, LAYER_STEP = 40, 2.0, 0.05


class _Soup:
    def __init__(self):
        self.pos, self.tri, self.flags, self.nv = [], [], [], 0

    def tris(self, p, t, flags=0):
        p = np.asarray(p, np.float64).reshape(-1, 3)
        t = np.asarray(t, np.int64).reshape(-1, 3)
        self.pos.append(p)
        self.tri.append(t + self.nv)
        self.flags.append(np.full(len(t), flags, np.uint32))
        self.nv += len(p)
        return len(t)

    def quad(self, origin, ex, ey, nx=1, ny=1, flags=0):
        """origin + s ex + t ey, nx x ny cells of two triangles, counter-clockwise seen from ex x ey."""
        o, ex, ey = (np.asarray(v, np.float64) for v in (origin, ex, ey))
        s, t = np.meshgrid(np.arange(nx + 1) / nx, np.arange(ny + 1) / ny, indexing="xy")
        p = o + s[..., None] * ex + t[..., None] * ey
        i = np.arange((nx + 1) * (ny + 1)).reshape(ny + 1, nx + 1)
        a, b, c, d = i[:-1, :-1], i[:-1, 1:], i[1:, 1:], i[1:, :-1]
        tri = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 2).reshape(-1, 3)
        return self.tris(p.reshape(-1, 3), tri, flags)

    def scene(self, name, pos, target):
        ind = np.concatenate(self.tri).astype(np.uint32)
        flg = np.concatenate(self.flags)
        return Scene(name, np.concatenate(self.pos).astype(np.float32), np.ascontiguousarray(ind),
                     np.ascontiguousarray(flg), dict(pos=list(pos), target=list(target), up=[0.0, 1.0, 0.0]))


def _facing_quad(b, z, cells):
    """A quad on the plane z = -z facing +z, wider than the 65 x 49 frustum there (tan: 0.76 x 0.57)."""
    h = np.ceil(z) + 1.0
    return b.quad((-h, -h, -z), (2 * h, 0, 0), (0, 2 * h, 0), cells, cells)


def layers():
    b = _Soup()
    for i in range(LAYER_COUNT):
        _facing_quad(b, LAYER_Z0 + LAYER_STEP * i, 4)
    return b.scene("layers", (0, 0, 0), (0, 0, -1))


def layers_tight():
    b = _Soup()
    z = np.float32(LAYER_Z0)
    for i in range(LAYER_COUNT):
        _facing_quad(b, float(z), 4)
        for _ in range(3):
            z = np.nextafter(z, np.float32(np.inf), dtype=np.float32)
    return b.scene("layers_tight", (0, 0, 0), (0, 0, -1))


COINCIDENT_COPIES = 9


def coincident():
    """Triangle order: copy 0 of the repeated quad, quad 0 of the stack, copy 1, quad 1, ..."""
    b = _Soup()
    for i in range(COINCIDENT_COPIES):
        _facing_quad(b, 3.0, 2)                 # 8 triangles, the same every time
        _facing_quad(b, 2.5 + 0.125 * i, 2)     # the stack: 2.5 .. 3.5, its fifth quad on the repeated one's plane
    return b.scene("coincident", (0, 0, 0), (0, 0, -1))


# axis_walls: primitive-id ranges of the room's five walls (each a 6 x 6 grid = 72 triangles, added first)
AXIS_WALLS = {"floor": 0, "ceiling": 1, "left": 2, "right": 3, "back": 4}
AXIS_WALL_TRIS = 72


def axis_walls():
    b = _Soup()
    x0, x1, y0, y1, z0, z1 = -2.0, 2.0, 0.0, 3.0, -10.0, 0.5
    b.quad((x0, y0, z1), (x1 - x0, 0, 0), (0, 0, z0 - z1), 6, 6)      # floor, facing +y
    b.quad((x0, y1, z0), (x1 - x0, 0, 0), (0, 0, z1 - z0), 6, 6)      # ceiling, facing -y
    b.quad((x0, y0, z1), (0, 0, z0 - z1), (0, y1 - y0, 0), 6, 6)      # left wall, facing +x
    b.quad((x1, y0, z0), (0, 0, z1 - z0), (0, y1 - y0, 0), 6, 6)      # right wall, facing -x
    b.quad((x0, y0, z0), (x1 - x0, 0, 0), (0, y1 - y0, 0), 6, 6)      # back wall, facing +z
    b.quad((0.5, 0.0, -6.0), (0, 0, 4.0), (0, 3.0, 0), 4, 4, FLAG_DOUBLE_SIDED)     # partition on x = 0.5
    b.quad((-2.0, 1.0, -3.0), (4.0, 0, 0), (0, 0, -4.0), 4, 4, FLAG_DOUBLE_SIDED)   # shelf on y = 1
    # steps against the back wall: faces on axis planes, edges on the camera's planes x = 0.5 and y = 1
    for k in range(4):
        zf, yt = -9.5 + 0.5 * k, 1.0 - 0.25 * k
        b.quad((0.5, 0.0, zf), (1.5, 0, 0), (0, yt, 0), 2, 2)                       # riser, facing +z
        b.quad((0.5, yt, zf), (1.5, 0, 0), (0, 0, -0.5), 2, 2)                      # tread, facing +y
    return b.scene("axis_walls", (0.5, 1.0, 0.0), (0.5, 1.0, -1.0))


def grazing():
    b = _Soup()
    b.quad((-256.0, 0.0, 16.0), (512.0, 0, 0), (0, 0, -528.0), 24, 24)              # floor, facing +y
    b.quad((-256.0, 0.0, -512.0), (512.0, 0, 0), (0, 64.0, 0), 8, 4)                # far wall, facing +z
    b.quad((-256.0, 0.0, 16.0), (0, 0, -528.0), (0, 64.0, 0), 8, 4)                 # left wall, facing +x
    b.quad((256.0, 0.0, -512.0), (0, 0, 528.0), (0, 64.0, 0), 8, 4)                 # right wall, facing -x
    # the view axis meets the floor at 0.5 degrees, 57 units ahead
    return b.scene("grazing", (0.0, 0.5, 0.0), (0.0, 0.5 - float(np.tan(np.radians(0.5))), -1.0))


SLIVER_COUNT = 1400


def slivers():
    """Needles of width 1/512 through the view axis: needle i spans the frustum at angle 137.5 i degrees, its ends
    up to 3 units apart in depth, so the boxes of neighbours in depth overlap and most rays cross most boxes
    without hitting the needle inside.  Every 20th needle is degenerate."""
    rng = np.random.default_rng(11)
    b = _Soup()
    for i in range(SLIVER_COUNT):
        z = 2.0 + 28.0 * i / SLIVER_COUNT
        ang = np.radians(137.5 * i)
        u = np.array([np.cos(ang), np.sin(ang), 0.0])
        v = np.array([-np.sin(ang), np.cos(ang), 0.0])
        reach = 0.9 * z + 0.5
        dz = rng.uniform(-1.5, 1.5)
        c = np.array([rng.uniform(-0.2, 0.2) * z, rng.uniform(-0.15, 0.15) * z, -z])
        p0, p1 = c - reach * u + (0, 0, dz), c + reach * u - (0, 0, dz)
        w = v / 512.0
        kind = i % 20
        if kind == 0:      # two equal vertices
            b.tris([p0, p1, p1], [[0, 1, 2]], FLAG_DOUBLE_SIDED)
        elif kind == 7:    # three collinear vertices
            b.tris([p0, 0.5 * (p0 + p1), p1], [[0, 1, 2]], FLAG_DOUBLE_SIDED)
        elif kind == 13:   # nearly no area: one float ulp wide at most
            b.tris([p0, p1, p1 + v * 1e-7], [[0, 1, 2]], FLAG_DOUBLE_SIDED)
        else:
            b.tris([p0 - w, p1 - w, p1 + w, p0 + w], [[0, 1, 2], [0, 2, 3]], FLAG_DOUBLE_SIDED)
    b.quad((-40.0, -40.0, -32.0), (80.0, 0, 0), (0, 80.0, 0), 4, 4)   # a backstop: every ray ends on a hit
    return b.scene("slivers", (0, 0, 0), (0, 0, -1))


BASE = {"layers": layers, "layers_tight": layers_tight, "coincident": coincident, "axis_walls": axis_walls,
        "grazing": grazing, "slivers": slivers}
NAMES = list(BASE) + [f"{k}_{n}" for k in OFFSETS for n in FAR_BASES]
_cache = {}


def translated(scene, offset, name):
    """`scene` and its camera moved by `offset`, the sums rounded to float32 (the float grid out there)."""
    off = np.asarray(offset, np.float32)
    cam = dict(scene.camera)
    for k in ("pos", "target"):
        cam[k] = [float(v) for v in (np.asarray(cam[k], np.float32) + off).astype(np.float32)]
    return dataclasses.replace(scene, name=name, positions=(scene.positions + off).astype(np.float32), camera=cam)


def make(name) -> Scene:
    if name not in _cache:
        if name in BASE:
            _cache[name] = BASE[name]()
        else:
            far, base = name[:5], name[6:]
            _cache[name] = translated(make(base), OFFSETS[far], name)
    return _cache[name]


def base_of(name):
    return name if name in BASE else name[6:]


def frame_config(N=16, max_count=64, impl=3, cull=1, **kw):
    """65 x 49, no guard bands, divisor 1, jitter off: SD texel (x, y) is pixel (x, y) and shares its ray."""
    from rsd.frame import FrameConfig
    return FrameConfig(visible_w=W, visible_h=H, guard_band=0, divisor=1, sd_guard_px=0, jitter=False,
                       sd_samples=N, max_count=max_count, implementation=impl, cull_mode=cull, numerics="exact", **kw)
