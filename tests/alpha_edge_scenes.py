"""Small scenes in which the rendered depth IS the alpha decision (tests/test_alpha_edges.py proves on the CPU that
each reaches its edges, tests/test_gpu_alpha_edges.py renders them): an opaque backdrop quad, and in front of it
alpha-masked double-sided cards of two triangles each that tile the view of a camera at the origin looking down -z.
A pixel shows the card's depth where alpha >= threshold and the backdrop's otherwise.  Textures are seeded 8-bit noise,
smoothed and stretched to the full range, so that many pixels lie near the threshold.  Texture coordinates are affine
per card.  All scenes stay inside the texcoord contract (include/rsd.h rsd_alpha_desc.texcoords).

build(name) returns (rsd.scenes.Scene, cards): cards is a list of Card with the two primitive ids of each card and
what is known about its decision without any sampler (`identity`)."""
import dataclasses
import math

import numpy as np

F = np.float32
NO_TEXTURE = 0xFFFFFFFF
FLAG_DOUBLE_SIDED, FLAG_ALPHA_MASK = 1, 4

VISIBLE = (160, 96)   # the largest frame the tests render: visible pixels ...
GUARD = 16            # ... plus this guard band for the LOD 0 consumers (192 x 128); the SD maps are 160 x 96
FOCAL, FRAME_HEIGHT = 21.0, 24.0
# the view's half extent in units of the distance: tan(fovY / 2) = 12 / 21 times the wider aspect (160 / 96), rounded up
HALF_X, HALF_Y = 1.0, 0.6

NAMES = ("shapes", "uv_domain", "lod_ladder", "thresholds")
LOD0_SCENES = ("shapes", "uv_domain", "thresholds")   # rendered by the consumers that test at LOD 0
CONE_SCENES = ("lod_ladder", "uv_domain")             # rendered by the SD trace (ray-cone LOD)
SHAPES = [(1, 1), (9, 1), (1, 9), (2, 2), (7, 5), (3, 16), (17, 33), (2, 255), (256, 256)]  # numpy (h, w): w x h below
# = 1x1, 1x9, 9x1, 2x2, 5x7, 16x3, 33x17, 255x2, 256x256 as width x height


@dataclasses.dataclass
class Card:
    name: str
    prims: tuple          # the card's two primitive ids
    material: int
    # None: both outcomes must occur.  "kept" / "discarded": the decision is the same for every hit and known without
    # a sampler (threshold 0, 1.5, NaN, constant alpha).  "constant": one value whatever the hit (a 1 x 1 texture, or
    # every hit past the last mip), kept or discarded as the sampler says
    identity: str | None = None


def noise(h, w, seed, passes=1, value=None, gain=1.0):
    """Seeded 8-bit noise with content at every scale -- one octave per mip size of the texture, each a coarse noise
    image enlarged to h x w, so that the deep mips still vary -- box-smoothed `passes` times over 3 x 3 wrapped texels
    where an axis has more than 2, centred on 127.5 (the mean of every mip stays near the 0.5 threshold) and
    stretched to the full range; gain > 1 stretches further and clips, which leaves plateaus of 0 and 255."""
    if value is not None:
        return np.full((h, w), value, np.uint8)
    rng = np.random.default_rng(seed)
    a = np.zeros((h, w))
    mh, mw = h, w
    while True:
        coarse = rng.integers(0, 256, (mh, mw)).astype(np.float64)
        a += coarse[(np.arange(h) * mh // h)[:, None], (np.arange(w) * mw // w)[None, :]]
        if (mh, mw) == (1, 1):
            break
        mh, mw = max(1, mh // 2), max(1, mw // 2)
    for _ in range(passes):
        if w > 2:
            a = (np.roll(a, 1, 1) + a + np.roll(a, -1, 1)) / 3.0
        if h > 2:
            a = (np.roll(a, 1, 0) + a + np.roll(a, -1, 0)) / 3.0
    a -= a.mean()
    if np.abs(a).max() > 0:
        a *= gain * 127.5 / np.abs(a).max()
    return np.clip(np.round(a + 127.5), 0, 255).astype(np.uint8)


class _Builder:
    def __init__(self, backdrop):
        self.pos, self.ind, self.flg, self.uv, self.mat, self.cards = [], [], [], [], [], []
        d = float(backdrop)
        self._quad([(-1.3 * d, -0.9 * d, -d), (1.3 * d, -0.9 * d, -d), (1.3 * d, 0.9 * d, -d), (-1.3 * d, 0.9 * d, -d)],
                   np.zeros((4, 2)), 0, 0)
        self.backdrop = d

    def _quad(self, corners, uv, flags, mat):
        n = len(self.pos)
        self.pos += [list(c) for c in corners]
        self.uv += [list(c) for c in uv]
        self.ind += [[n, n + 1, n + 2], [n, n + 2, n + 3]]
        self.flg += [flags, flags]
        self.mat += [mat, mat]
        return (len(self.ind) - 2, len(self.ind) - 1)

    def card(self, name, cell, grid, dist, mat, uv_origin, uv_ds, uv_dt, tilt=0.0, identity=None):
        """The card of grid cell (i, j) of (nx, ny) at distance `dist`, turned by `tilt` radians about the vertical
        axis through its centre; uv = uv_origin + s uv_ds + t uv_dt over the card's (s, t) in [0, 1]^2."""
        (i, j), (nx, ny) = cell, grid
        x0, x1 = -HALF_X + 2 * HALF_X * i / nx, -HALF_X + 2 * HALF_X * (i + 1) / nx
        y0, y1 = -HALF_Y + 2 * HALF_Y * j / ny, -HALF_Y + 2 * HALF_Y * (j + 1) / ny
        cx, cz = 0.5 * (x0 + x1) * dist, -dist
        c, s = math.cos(tilt), math.sin(tilt)
        corners = []
        for (x, y) in ((x0, y0), (x1, y0), (x1, y1), (x0, y1)):
            dx = x * dist - cx
            corners.append((cx + c * dx, y * dist, cz + s * dx))
        o, a, b = (np.asarray(v, np.float64) for v in (uv_origin, uv_ds, uv_dt))
        uv = [o, o + a, o + a + b, o + b]
        prims = self._quad(corners, uv, FLAG_DOUBLE_SIDED | FLAG_ALPHA_MASK, mat)
        self.cards.append(Card(name, prims, mat, identity))

    def build(self, name, materials, textures):
        from rsd.scenes import AlphaMaterials, Scene
        m = [(0.5, 1.0, NO_TEXTURE)] + list(materials)  # material 0: the backdrop
        am = AlphaMaterials(np.array(self.uv, F), np.array(self.mat, np.uint32), np.array([x[0] for x in m], F),
                            np.array([x[1] for x in m], F), np.array([x[2] for x in m], np.uint32), textures)
        cam = {"pos": [0.0, 0.0, 0.0], "target": [0.0, 0.0, -1.0], "up": [0.0, 1.0, 0.0]}
        return Scene(name, np.array(self.pos, F), np.array(self.ind, np.uint32), np.array(self.flg, np.uint32), cam,
                     am), self.cards


def _shapes():
    """Nine textures in one table, one card each: the texel offsets and mip counts of a long table.  Every card's
    texture coordinates straddle the wrap seam of both axes and span about ten texels, or 1.5 periods of a smaller
    texture, slightly sheared so that no row or column of pixels shares a coordinate (a card aligned with the pixel grid
    has one v per row: 128 values, among which a fraction that rounds to 256 / 256 need not occur)."""
    B = _Builder(12.0)
    textures = [noise(h, w, 100 + k, passes=1 if max(h, w) < 64 else 2, value=140 if (h, w) == (1, 1) else None)
                for k, (h, w) in enumerate(SHAPES)]
    assert sum(t.size for t in textures) < 70 * 1024
    mats = [(0.5, 1.0, k) for k in range(len(SHAPES))]
    for k, (h, w) in enumerate(SHAPES):
        wu, wv = min(1.5, 10.0 / w), min(1.5, 10.0 / h)
        B.card(f"{w}x{h}", (k % 3, k // 3), (3, 3), 6.0 + 0.05 * k, 1 + k, (-0.4 * wu, -0.45 * wv), (wu, 0.013 * wv), (-0.017 * wu, wv),
               identity="constant" if (h, w) == (1, 1) else None)
    return B.build("shapes", mats, textures)


def _uv_domain():
    """Six cards of an 8 x 8 and a 5 x 7 texture at distance 16, where the ray cone's level lies inside their chains
    (0.6 to 1.4 and 0.2 to 1.0 from the view's centre to its corners)."""
    B = _Builder(32.0)
    textures = [noise(8, 8, 201), noise(7, 5, 202)]
    mats = [(0.5, 1.0, 0), (0.5, 1.0, 1)]
    g, d = (3, 2), 16.0
    B.card("negative", (0, 0), g, d, 1, (-3.2, -2.6), (1.5, 0.02), (-0.03, 1.5))
    B.card("tiled 7.5", (1, 0), g, d, 2, (0.0, 0.0), (7.5, 0.1), (-0.15, 7.5))
    B.card("0 and 1", (2, 0), g, d + 0.5, 1, (0.0, 0.0), (1.0, 0.0), (0.0, 1.0))
    B.card("near 1000", (0, 1), g, d + 0.5, 2, (999.0, -1000.75), (1.5, 0.02), (-0.03, 1.5))
    B.card("mirrored", (1, 1), g, d, 1, (1.3, 0.1), (-1.5, 0.02), (0.03, 1.5))
    B.card("sheared", (2, 1), g, d, 2, (0.05, 0.1), (1.5, 0.4), (-0.3, 3.2))
    return B.build("uv_domain", mats, textures)


def ray_cone_spread(height=VISIBLE[1]):
    """The value of rsd_ray_cone_spread(FOCAL, height) to the precision a generator needs."""
    fov = 2.0 * math.atan(0.5 * FRAME_HEIGHT / FOCAL)
    return round(math.atan(2.0 * math.tan(fov / 2.0) / height), 6)


# the levels the ladder's flat cards are placed at, per texture (numpy shape): below level 0, inside every mip
# interval, past the last mip (64 x 64: 7 mips, 5 x 7: 3 mips)
LADDER = {(64, 64): [-0.8, 0.45, 1.5, 2.45, 3.5, 4.55, 5.25, 6.6], (7, 5): [-0.6, 0.5, 1.2, 2.5],
          (3, 16): [0.5, 1.5, 2.5]}  # 16 x 3: 8 x 1, 4 x 1, 2 x 1, 1 x 1 -- the height reaches 1 three mips before the width
LADDER_TILTED = [((64, 64), 1.0, 0.9), ((7, 5), 0.9, 0.8), ((64, 64), 5.3, 0.6)]  # (texture, level untilted, tilt)


def _lod_ladder():
    """For the SD trace (ray-cone LOD): cards of one 64 x 64, one 5 x 7 and one 16 x 3 texture at the distances where a ray down
    the view axis has the levels of LADDER, three of them tilted (the level rises by log2(1 / |d . n|) across them)."""
    spread = ray_cone_spread()
    shapes = list(LADDER)
    dist = lambda shape, level: 2.0 ** (level - 0.5 * math.log2(shape[0] * shape[1])) / spread  # noqa: E731
    far = max(dist(s, l) for s in shapes for l in LADDER[s])
    B = _Builder(2.0 * far)
    textures = [noise(64, 64, 301, passes=2), noise(7, 5, 304), noise(3, 16, 305)]
    mats = [(0.5, 1.0, 0), (0.5, 1.0, 1), (0.5, 1.0, 2)]
    todo = [(s, l, 0.0) for s in shapes for l in LADDER[s]] + LADDER_TILTED
    g = (6, 3)
    assert len(todo) == g[0] * g[1]
    for k, (s, level, tilt) in enumerate(todo):
        ti = shapes.index(s)
        h, w = s
        past = tilt == 0.0 and level > len(_chain_sizes(h, w)) - 1
        # a dozen texels of the mip the card mostly reads across the card, or 1.5 periods of a mip of 8 texels or fewer
        mw, mh = max(1, w >> max(0, int(level))), max(1, h >> max(0, int(level)))
        wu, wv = 12.0 / mw if mw > 8 else 1.5, 12.0 / mh if mh > 8 else 1.5
        B.card(f"{w}x{h} level {level:g}" + (f" tilt {tilt:g}" if tilt else ""), (k % g[0], k // g[0]), g,
               dist(s, level), 1 + ti, (-0.37 * wu, -0.41 * wv), (wu, 0.013 * wv), (-0.017 * wu, wv), tilt=tilt,
               identity="constant" if past else None)
    return B.build("lod_ladder", mats, textures)


def _chain_sizes(h, w):
    out = [(h, w)]
    while out[-1] != (1, 1):
        out.append((max(1, out[-1][0] // 2), max(1, out[-1][1] // 2)))
    return out


def _thresholds():
    """Constant-alpha and textured materials at the thresholds' edges, one card each."""
    B = _Builder(12.0)
    textures = [noise(16, 16, 401, gain=1.6), noise(4, 4, 0, value=255)]  # plateaus of 255: alpha 1.0 occurs
    nan = float("nan")
    h33, h77 = F(np.float16(0.33)), F(np.float16(0.7777))
    below = lambda x: float(np.nextafter(x, F(-1)))  # noqa: E731
    table = [  # (name, threshold, constant alpha, texture, identity)
        ("threshold 0", 0.0, 1.0, 0, "kept"),
        ("threshold 1.0, all 255", 1.0, 1.0, 1, "kept"),
        ("threshold 1.0", 1.0, 1.0, 0, None),
        ("threshold 1.5", 1.5, 1.0, 0, "discarded"),
        ("threshold 0.33", 0.33, 1.0, 0, None),
        ("threshold 0.7777", 0.7777, 1.0, 0, None),
        ("alpha = half(0.33)", 0.33, float(h33), NO_TEXTURE, "kept"),
        ("alpha below half(0.33)", 0.33, below(h33), NO_TEXTURE, "discarded"),
        ("alpha = half(0.7777)", 0.7777, float(h77), NO_TEXTURE, "kept"),
        ("alpha below half(0.7777)", 0.7777, below(h77), NO_TEXTURE, "discarded"),
        ("NaN alpha", 0.5, nan, NO_TEXTURE, "kept"),
        ("NaN threshold", nan, 1.0, 0, "kept"),
    ]
    g = (4, 3)
    for k, (name, thr, al, tex, ident) in enumerate(table):
        B.card(name, (k % g[0], k // g[0]), g, 6.0 + 0.05 * k, 1 + k, (-0.21, -0.17), (1.3, 0.011), (-0.014, 1.3),
               identity=ident)
    return B.build("thresholds", [(t[1], t[2], t[3]) for t in table], textures)


_BUILDERS = {"shapes": _shapes, "uv_domain": _uv_domain, "lod_ladder": _lod_ladder, "thresholds": _thresholds}
_cache = {}


def build(name):
    if name not in _cache:
        scene, cards = _BUILDERS[name]()
        for a in (scene.positions, scene.indices, scene.flags, scene.alpha.texcoords, scene.alpha.tri_material):
            a.setflags(write=False)
        _cache[name] = (scene, cards)
    return _cache[name]


def identity_variant(scene, cards):
    """The scene the identities promise: every "kept" card opaque (its alpha bit cleared), every "discarded" card
    removed; the other cards as they are."""
    flags = scene.flags.copy()
    keep = np.ones(scene.indices.shape[0], bool)
    for c in cards:
        if c.identity == "kept":
            flags[list(c.prims)] &= ~np.uint32(FLAG_ALPHA_MASK)
        elif c.identity == "discarded":
            keep[list(c.prims)] = False
    am = dataclasses.replace(scene.alpha, tri_material=np.ascontiguousarray(scene.alpha.tri_material[keep]))
    return dataclasses.replace(scene, indices=np.ascontiguousarray(scene.indices[keep]),
                               flags=np.ascontiguousarray(flags[keep]), alpha=am)


def opaque_variant(scene):
    """Every card opaque: no alpha data at all."""
    return dataclasses.replace(scene, alpha=None)


def moved(scene, step):
    """The positions with every card translated by its own small offset of `step` (1, 2, ...); the backdrop stays.
    The cards stay in front of the backdrop and go on covering most of their cells."""
    p = scene.positions.copy()
    rng = np.random.default_rng(1000 + step)
    depth = -float(scene.positions[0, 2])  # the backdrop's distance
    for q in range(1, scene.positions.shape[0] // 4):
        d = -float(scene.positions[4 * q, 2])
        off = rng.uniform(-1.0, 1.0, 3) * np.array([0.04 * d, 0.04 * d, min(0.1 * d, 0.2 * (depth - d))])
        p[4 * q:4 * q + 4] += off.astype(F)
    return np.ascontiguousarray(p, F)


def frame_config(guard=GUARD, **kw):
    """The frame of the LOD 0 consumers (guard band 16) or, with guard=0, of the SD maps: divisor 1, no SD guard band,
    no jitter, N = 4."""
    from rsd.frame import FrameConfig
    args = dict(visible_w=VISIBLE[0], visible_h=VISIBLE[1], guard_band=guard, divisor=1, sd_samples=4, max_count=8,
                sd_guard_px=0, jitter=False, cull_mode=0, focal_length=FOCAL, frame_height=FRAME_HEIGHT, numerics="exact")
    args.update(kw)
    return FrameConfig(**args)


# ---- what the CPU and the GPU file share to render the scenes

def oscene(oracle, scene):
    return oracle.Scene(scene.positions, scene.indices, scene.flags, scene.alpha)


def camera(oracle, cfg):
    """(librsd's camera, the oracle's) of a frame of cfg: at the origin, looking down -z."""
    from helpers import to_oracle
    from rsd.frame import look_at
    cam = look_at([0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0], cfg)
    return cam, to_oracle(cam, oracle.Camera)


def sd_params(oracle, impl=3, alpha_test=1, hit_order=0, N=4, max_count=8, cull=0):
    """The SD trace driven directly from the camera: no guard band, no jitter, no intervals, normalised depths."""
    return oracle.SDParams(N, impl, max_count, 0, 0, 1, 0, cull, alpha_test, float(F(1.5 / N)), hit_order, 0)
