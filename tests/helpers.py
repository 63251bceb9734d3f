"""Shared test helpers: struct conversion between librsd and the oracle, the oracle side of a whole
frame (G-buffer -> pass 1 -> SD trace -> pass 2), the SVAO parameter sweep of test_svao_params.py /
test_gpu_svao_params.py, the frames of odd geometry of test_odd_geometry.py / test_gpu_odd_geometry.py, the shapes,
inputs and canary buffers of test_odd_passes.py / test_gpu_odd_passes.py (the passes outside the SVAO frame), and the
grading of a fast-numerics frame against the exact oracle (test_gpu_numerics.py, test_gpu_svao_params.py)."""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import NamedTuple

import numpy as np


def to_oracle(struct, oracle_cls):
    """Byte-copy a librsd ctypes struct into the oracle's struct of identical layout.  The oracle's
    struct may be a prefix of librsd's (device-only trailing fields such as rsd_svao_params.tile_flags)."""
    out = oracle_cls()
    names = [f[0] for f in type(struct)._fields_]
    # a field the oracle does not use keeps librsd's name with an "_unused" suffix
    onames = [f[0].removesuffix("_unused") for f in oracle_cls._fields_]
    names = [n.removeprefix("d_") for n in names]  # librsd's device pointers vs the oracle's host pointers
    assert names[:len(onames)] == onames, (oracle_cls, onames, names)
    assert C.sizeof(out) <= C.sizeof(struct), (oracle_cls, C.sizeof(out), C.sizeof(struct))
    C.memmove(C.byref(out), C.byref(struct), C.sizeof(out))
    return out


def oracle_vao(O, fb_w, fb_h, divisor, sd_guard_px=512, radius=0.2, exponent=2.0, thickness=0.0):
    """SVAO::compile restated independently (SVAO.cpp:143-150, 700-723)."""
    v = O.VAOData()
    v.resolution[:] = [fb_w, fb_h]
    v.invResolution[0] = float(np.float32(1.0) / np.float32(fb_w))
    v.invResolution[1] = float(np.float32(1.0) / np.float32(fb_h))
    v.sdGuard = sd_guard_px // divisor
    low = ((fb_w + divisor - 1) // divisor, (fb_h + divisor - 1) // divisor) if divisor > 1 else (fb_w, fb_h)
    v.lowResolution[:] = low
    v.noiseScale[:] = [float(np.float32(fb_w) / np.float32(4)), float(np.float32(fb_h) / np.float32(4))]
    v.radius, v.exponent, v.thickness = radius, exponent, thickness
    v.ssRadiusCutoff, v.ssMaxRadius = 6.0, 512.0
    return v, low[0] + 2 * v.sdGuard, low[1] + 2 * v.sdGuard


def oracle_frame(O, oscene, cam, vao, sdp, svp, fb_w, fb_h, sd_w, sd_h, threads=None):
    z, n = O.gbuffer(oscene, cam, fb_w, fb_h, sdp.cull_mode, threads=threads)
    ao1, st, rmin, rmax = O.svao_pass1(cam, vao, svp, z, n, sd_w, sd_h)
    sd, stats = O.sd_trace(oscene, cam, sdp, z, rmin, rmax, sd_w, sd_h, threads=threads)
    ao2 = O.svao_pass2(cam, vao, svp, z, n, st, sd, ao1, threads=threads)
    return dict(depth=z, normals=n, ao1=ao1, stencil=st, ray_min=rmin, ray_max=rmax, sd=sd, ao=ao2, stats=stats)


def small_frame_config(visible=(160, 96), guard=16, divisor=2, N=4, max_count=8, impl=0, radius=1.0):
    """A small frame; the AO radius is scaled up so that, at this resolution, the sample
    radius exceeds ssRadiusCutoff (6 px) and pass 1 actually requests SD rays."""
    from rsd.frame import FrameConfig
    return FrameConfig(visible_w=visible[0], visible_h=visible[1], guard_band=guard, divisor=divisor,
                       sd_samples=N, max_count=max_count, implementation=impl, sd_guard_px=64, radius=radius)


# ---- the SVAO parameter sweep (test_svao_params.py checks on the oracle alone that every point reaches
# the branches it is meant to reach; test_gpu_svao_params.py runs the kernels at the same points)

# (exponent, thickness, ssMaxRadius, ssRadiusCutoff, radius): the point every other test runs at ...
SVAO_DEFAULT_POINT = (2.0, 0.0, 512.0, 6.0, 1.0)
# ... and the points away from it.  ssMaxRadius = 24 clamps the screen radius of the pixels nearest the
# camera (basic_init shrinks the pixel's AO radius; sample_init leaves the host-evaluated direction terms)
SVAO_SWEEP = [
    (1.5, 0.5, 512.0, 6.0, 1.0),
    (3.0, 1.0, 24.0, 6.0, 1.0),
    (0.5, 0.25, 48.0, 12.0, 1.0),
    (1.0, 0.0, 24.0, 6.0, 4.0),
    (2.0, 2.0, 512.0, 6.0, 1.0),
]
# the sweep points whose ssMaxRadius must clamp a good part of the frame, and leave a good part unclamped
SVAO_CLAMPED_POINTS = (1, 3)
SVAO_SMALL_VISIBLE = (160, 96)    # the sweep's frame: guard 16, divisor 2, N = 4 (small_frame_config)
SVAO_RAGGED_VISIBLE = (200, 120)  # ... and a visible size that is no multiple of the 16 / 32-pixel tiles


def svao_point_id(point):
    return "e{:g}_t{:g}_max{:g}_cut{:g}_r{:g}".format(*point)


def svao_point_config(point, visible=SVAO_SMALL_VISIBLE, divisor=2, **kw):
    """The sweep's small frame at `point`: exponent, thickness and radius travel in the FrameConfig."""
    import dataclasses
    exponent, thickness, _, _, radius = point
    return dataclasses.replace(small_frame_config(visible=visible, guard=16, divisor=divisor, N=4, radius=radius),
                               exponent=exponent, thickness=thickness, **kw)


def set_svao_point(vao, point):
    """Write a sweep point into a VAOData (librsd's or the oracle's: the same public fields)."""
    vao.exponent, vao.thickness, vao.ssMaxRadius, vao.ssRadiusCutoff, vao.radius = point
    return vao


def radius_in_pixels(cam, vao, depth):
    """BasicAOData::Init's screen-space radius of every pixel before the ssMaxRadius clamp
    (Common.slang:296-303), in float32 operation by operation; a pixel is clamped where it exceeds
    vao.ssMaxRadius."""
    f = np.float32
    z = np.asarray(depth, np.float32)
    rf = f(vao.radius) * f(cam.focalLength)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pa = rf / (f(cam.frameWidth) * z) * f(vao.resolution[0])
        pb = rf / (f(cam.frameHeight) * z) * f(vao.resolution[1])
        return pa + f(0.5) * (pb - pa)


# ---- frames of odd geometry (test_odd_geometry.py checks on the oracle alone that each of them reaches the
# branches it is meant to reach; test_gpu_odd_geometry.py runs the kernels on them)

class OddFrame(NamedTuple):
    name: str
    visible_w: int
    visible_h: int
    guard: int
    divisor: int
    sd_guard_px: int
    radius: float


# arcade_tiny with its own camera, N = 4, max_count 8
ODD_FRAMES = [
    # odd prime width, odd guard band, divisor 3, sdGuard = 7 / 3 = 2, SD map 60 x 39
    OddFrame("odd_div3", 157, 93, 5, 3, 7, 1.0),
    # ceil(fb / 4): 111 x 75 -> 28 x 19, sdGuard 3, SD map 34 x 25
    OddFrame("odd_div4", 97, 61, 7, 4, 13, 2.0),
    # no guard band and sdGuard 0 (the generic pass 1), SD map 66 x 34
    OddFrame("no_guards", 131, 67, 0, 2, 0, 2.0),
    # smaller than one 32 x 32 pass-1 workgroup and than one 64-lane wave row; SD map 17 x 13
    OddFrame("tiny", 20, 12, 3, 2, 5, 2.0),
    # one pixel above a multiple of 32 in both axes (the last 32-row group holds one visible row), a one-pixel guard
    # band, full-resolution SD map 105 x 73.  (65 x 33 with radius 4 stencils 1009 visible pixels, too close to the
    # 1000 that test_odd_geometry.py asks for; this one 2879.)
    OddFrame("one_over", 97, 65, 1, 1, 3, 3.0),
]
# the SD map sizes the shapes are meant to have: lowResolution = ceil(fb / divisor), sdGuard = sd_guard_px // divisor
ODD_SD_SIZES = {"odd_div3": (60, 39), "odd_div4": (34, 25), "no_guards": (66, 34), "tiny": (17, 13),
                "one_over": (105, 73)}


# ---- shapes of the passes outside the SVAO frame (test_odd_passes.py checks on the checkers alone that each of them
# can show a fault; test_gpu_odd_passes.py runs the kernels on them)

# (W, H) for the kernels with an 8 x 8 tile and one lane per pixel (rsd_gbuffer_raster, rsd_gbuffer_world,
# rsd_depth_peel, rsd_rtao, rsd_sd_raster): one pixel, below a tile on both axes, exactly one tile, one over, one over
# eight tiles and one over two.  W * H = 1, 21, 64, 81, 1105 around the 256 lanes of the flat kernels
PIXEL_SHAPES = [(1, 1), (7, 3), (8, 8), (9, 9), (65, 17)]
# (W, H) of the full-resolution frame for the kernels with a 64 x 4 block.  rsd_hbao works on 16 layers of
# ceil(W / 4) x ceil(H / 4): 1 x 1 layers (at (3, 2) ten of the sixteen hold no pixel of the image), 2 x 2 layers,
# layers of exactly one block, layers of 65 x 5
BLOCK_SHAPES = [(1, 1), (3, 2), (5, 7), (256, 16), (257, 17)]
# (W, H, guard band) for rsd_hbao, whose scissor on the layers is guard_band / 4: both guard bands of the existing
# tests wherever they leave a texel inside the scissor ...
HBAO_SHAPES = [(w, h, g) for w, h in BLOCK_SHAPES for g in (0, 8)
               if (w + 3) // 4 > 2 * (g // 4) and (h + 3) // 4 > 2 * (g // 4)]
# ... a scissor of 2 x -2 texels (nothing may be drawn) and a scissor of one texel per layer
HBAO_EMPTY_SCISSOR = (40, 24, 16)
HBAO_ONE_TEXEL_SCISSOR = (44, 44, 20)
# rsd_temporal_depth_peel works at full resolution: the same sizes, and exactly one block and one over
TEMPORAL_PEEL_SHAPES = BLOCK_SHAPES + [(64, 4), (65, 5)]


# The camera of the tile kernels at PIXEL_SHAPES, for the opaque and the alpha scene of depth_peel_checker alike: from
# a corner of the hall across its props, farZ pulled in (as tests/test_gpu_rtao.py does with CLIP_FAR) so that the
# G-buffer misses a good part of every frame, the centre pixel -- the 1 x 1 frame -- hits, and a second layer lies
# behind a good part of the hits; ODD_PASS_RTAO_MAX_T lets about a fifth of the spp = 1 rays hit.  Found by a search
# over poses on the checkers alone; tests/test_odd_passes.py asserts the conditions.
ODD_PASS_CAMERA = dict(pos=[14.93, 3.29, 10.8], target=[-8.88, 1.54, 1.21], up=[0.0, 1.0, 0.0])
ODD_PASS_FAR = 18.0
ODD_PASS_RTAO_MAX_T = 6.0
# sd_raster_checker.BASE's AO radius is 6 on a 75 x 45 frame; these frames are up to five times smaller, and the
# radius in pixels shrinks with them: 24 keeps pass 1 requesting SD rays (an interval and a stencil) on all of them
ODD_PASS_SD_RADIUS = 24.0
ODD_PASS_SD_DIVISORS = (1, 2, 3)
ODD_PASS_SD_SAMPLES = (1, 4, 16)


def odd_pass_case(oracle, checker_module, kind, size):
    """checker_module.Case of `kind` at `size` seen by ODD_PASS_CAMERA with farZ = ODD_PASS_FAR (depth_peel_checker
    and rtao_checker); sd_raster_checker's alpha case keeps its own BASE_CAMERA."""
    from rsd.frame import look_at
    c = checker_module.Case(oracle, kind, size)
    if checker_module.__name__ != "sd_raster_checker":
        c.cam = look_at(ODD_PASS_CAMERA["pos"], ODD_PASS_CAMERA["target"], ODD_PASS_CAMERA["up"], c.cfg)
        c.cam.farZ = ODD_PASS_FAR
        c.ocam = to_oracle(c.cam, oracle.Camera)
    return c


def hbao_odd_input(HB, width, height):
    """hbao_checker.synthetic at a BLOCK_SHAPES size with a depth-0 patch that leaves most of a small frame alone,
    and the radius of the parity test there: 1 from 16 rows on (every texel above one pixel, hbao_checker.radii),
    16 / height below, which keeps 0.875 radius height / z >= 14 / 12 pixels."""
    s = HB.synthetic(width, height, zero_patch=min(16, max(1, min(width, height) // 4)))
    return s, max(1.0, 16.0 / height)


def restride(image, stride):
    """What a kernel that stored pixel (x, y) at y * stride + x would leave in the row-major buffer of `image`
    (H x W x ...): the mutant "row stride taken from the padded width".  Elements past the buffer are dropped (the
    canary's), elements never written are zero."""
    h, w = image.shape[:2]
    flat = np.zeros((max(h * stride, h * w),) + image.shape[2:], image.dtype)
    for y in range(h):
        flat[y * stride:y * stride + w] = image[y]
    return flat[:h * w].reshape(image.shape)


def roundup(v, m):
    return -(-v // m) * m


# rsd_rtao_pack: counts around its 256-lane block and the largest PIXEL_SHAPES frame
PACK_COUNTS = [1, 255, 256, 257, 1105]
PACK_SPECIALS = [np.nan, np.inf, 65520.0, 70000.0, -0.0]  # in the distance input: NaN, +inf, above 65504, -0


def pack_inputs(count):
    """(ambient in [0, 1], ray distance) of `count` elements; the distances start with as many of PACK_SPECIALS as
    fit, then 65504 and the float just below 65520 (both round to 65504) where there is room."""
    rng = np.random.default_rng(count)
    amb = rng.random(count).astype(np.float32)
    amb[:2] = [0.0, 1.0][:min(2, count)]
    dist = rng.uniform(0.0, 12.0, count).astype(np.float32)
    special = np.array(PACK_SPECIALS + [65504.0, np.nextafter(np.float32(65520.0), np.float32(0.0))], np.float32)
    n = min(count, len(special))
    dist[:n] = special[:n]
    return amb, dist


def pack_expected(amb, dist):
    """floor(255 a + 0.5) and numpy's float16 rounding (round to nearest even), as tests/test_gpu_rtao.py's
    test_graph states them; the float16 as its bits."""
    with np.errstate(over="ignore"):
        return (np.floor(amb.astype(np.float64) * 255.0 + 0.5).astype(np.uint8),
                dist.astype(np.float16).view(np.uint16))


def shape_id(s):
    return "x".join(str(v) for v in s[:2]) + "".join(f"_g{v}" for v in s[2:])


def band_rows(f, band_count):
    """The 32-row groups of the visible rows and the 8-row tile rows of the SD map of the odd frame f, dealt to
    band_count bands as rsd.h's band calls deal them (group g to band g % band_count): per band
    (groups, SD tile rows)."""
    sd_h = -(-(f.visible_h + 2 * f.guard) // f.divisor) + 2 * (f.sd_guard_px // f.divisor)
    groups, tiles = range(-(-f.visible_h // 32)), range(-(-sd_h // 8))
    return [([g for g in groups if g % band_count == b], [t for t in tiles if t % band_count == b])
            for b in range(band_count)]


def band_counts(f):
    """The band counts the band tests run the odd frame f at: 2, 3 and one more than it has 32-row groups, which
    leaves the last band without a row of pass 1 / pass 2."""
    return [2, 3, -(-f.visible_h // 32) + 1]


# ---- canaries: output buffers in the middle of a larger allocation of sentinel bytes

SENTINEL = 0xA5      # every byte of the padding and of a pre-filled buffer
PAD_ELEMENTS = 64    # at least this many elements of sentinel on either side of a view


class Canary:
    """A tensor of `shape` and `dtype` in the middle of a larger allocation full of sentinel bytes."""

    def __init__(self, torch, shape, dtype, device):
        item = torch.empty((), dtype=dtype).element_size()
        self.n = int(np.prod(shape)) * item
        self.pad = -(-PAD_ELEMENTS * item // 256) * 256   # a multiple of 256 bytes: the view keeps torch's alignment
        self.raw = torch.full((self.n + 2 * self.pad,), SENTINEL, dtype=torch.uint8, device=device)
        self.view = self.raw[self.pad:self.pad + self.n].view(dtype).view(tuple(shape))
        assert self.view.data_ptr() == self.raw.data_ptr() + self.pad and self.pad >= PAD_ELEMENTS * item

    def fill(self):
        self.raw.fill_(SENTINEL)

    def intact(self):
        return bool((self.raw[:self.pad] == SENTINEL).all()) and bool((self.raw[self.pad + self.n:] == SENTINEL).all())

    def numpy(self):
        """The view's content on the host (a copy)."""
        return self.view.cpu().numpy()

    def untouched(self):
        """Every byte of the view itself still holds the sentinel."""
        return bool((self.raw[self.pad:self.pad + self.n] == SENTINEL).all())


def sentinel_array(shape, dtype):
    """The host twin of a pre-filled buffer."""
    dtype = np.dtype(dtype)
    return np.full(tuple(shape[:-1]) + (shape[-1] * dtype.itemsize,), SENTINEL, np.uint8).view(dtype)


def canary(torch, shape, dtype, device="cuda"):
    """A canary view of `shape` and `dtype`, pre-filled with the sentinel like its padding."""
    return Canary(torch, shape, dtype, device)


def assert_canaries_intact(torch, canaries, stage):
    """After the work on the device has finished: no canary of the dict `canaries` (name -> Canary) has lost a
    sentinel byte of its padding."""
    torch.cuda.synchronize()
    for name, c in canaries.items():
        assert c.intact(), f"{stage}: a store outside the {name} buffer"


def odd_second_pose(scene):
    """A second camera pose of the scene (pos, target, up), far enough from its own for other SD texels to be
    touched: the clean-tile tests' second frame."""
    c = scene.camera
    return ([c["pos"][0] + 1.5, c["pos"][1] + 0.25, c["pos"][2] - 2.0],
            [c["target"][0] - 2.0, c["target"][1], c["target"][2]], list(c["up"]))


def odd_frame(name):
    return next(f for f in ODD_FRAMES if f.name == name)


def odd_frame_config(f, N=4, max_count=8, **kw):
    from rsd.frame import FrameConfig
    return FrameConfig(visible_w=f.visible_w, visible_h=f.visible_h, guard_band=f.guard, divisor=f.divisor,
                       sd_samples=N, max_count=max_count, sd_guard_px=f.sd_guard_px, radius=f.radius, **kw)


def right_bottom_guard(cfg):
    """A boolean image of the frame: the pixels of the right and bottom guard band, which pass 1's padded
    dispatch (roundup32 of the visible size from the first visible pixel) reaches and the left / top band not."""
    m = np.zeros((cfg.fb_h, cfg.fb_w), bool)
    if cfg.guard_band:
        m[cfg.fb_h - cfg.guard_band:, :] = True
        m[:, cfg.fb_w - cfg.guard_band:] = True
    return m


# ---- fast numerics graded against the exact oracle

AO_MAE = 1.0 / 255.0   # mean absolute AO error over the visible pixels
AO_P2 = 2              # ... and |diff| <= 2/255 ...
AO_P2_FRAC = 0.995     # ... on at least 99.5 % of them
DECISION_FRAC = 0.01   # stencil pixels / touched SD texels allowed to flip (reported; measured far below)


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def visible_region(cfg):
    return slice(cfg.guard_band, cfg.fb_h - cfg.guard_band), slice(cfg.guard_band, cfg.fb_w - cfg.guard_band)


def ao_stats(a, b, gv, mask=None):
    """AO difference in 1/255 units over the visible pixels (both channels with dualAO); mask: a boolean
    image of the visible region's shape selecting a subset of them."""
    d = np.abs(a[gv].astype(np.int32) - b[gv].astype(np.int32))
    if mask is not None:
        d = d[mask]
    return {"mae": float(d.mean()) / 255.0, "frac_le2": float((d <= AO_P2).mean()), "max": int(d.max()),
            "frac_exact": float((d == 0).mean())}


def check_ao(s, what):
    assert s["mae"] <= AO_MAE, (what, s)
    assert s["frac_le2"] >= AO_P2_FRAC, (what, s)


def report(case, **kw):
    """RSD_NUMERICS_REPORT=<path>: the measured figures of a case, appended there as a JSON line."""
    path = os.environ.get("RSD_NUMERICS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(case=case, **kw)) + "\n")


def grade(oracle, r, scene, case, detail=None):
    """One fast frame of renderer r (G-buffer already rendered) graded against the oracle.
    detail: a dict that receives the GPU frame ("gpu"), the oracle's exact AO of the same G-buffer
    ("ao") and the visible region ("gv"), for a caller that grades subsets of the pixels as well."""
    import torch
    cfg = r.cfg
    assert r.svp.numerics == 0, "the renderer must run the fast numerics"
    r.clear_intervals()
    r.pass1()
    torch.cuda.synchronize()
    ao1_g = r.ao.cpu().numpy().copy()
    r.sd_trace()
    r.pass2()
    g = r.numpy()
    cam, vao = to_oracle(r.cam, oracle.Camera), to_oracle(r.vao, oracle.VAOData)
    sdp, svp = to_oracle(r.sdp, oracle.SDParams), to_oracle(r.svp, oracle.SVAOParams)
    osc = oracle.Scene(scene.positions, scene.indices, scene.flags, scene.alpha)
    gv = visible_region(cfg)

    # the exact frame of the oracle on the same G-buffer
    ao1, st, rmin, rmax = oracle.svao_pass1(cam, vao, svp, g["depth"], g["normals"], r.sd_w, r.sd_h)
    sd, _ = oracle.sd_trace(osc, cam, sdp, g["depth"], rmin, rmax, r.sd_w, r.sd_h)
    ao = oracle.svao_pass2(cam, vao, svp, g["depth"], g["normals"], st, sd, ao1)
    frame = ao_stats(g["ao"], ao, gv)
    if detail is not None:
        detail.update(gpu=g, ao=ao, gv=gv)

    # pass-1 decisions
    stencil_flip = float((g["stencil"][gv] != st[gv]).mean())
    touched_g = (g["ray_max"] != 0)
    touched_o = (rmax != 0)
    touched_flip = float((touched_g != touched_o).sum() / max(1, touched_o.sum()))
    both = touched_g & touched_o
    iv_differ = float(((g["ray_min"] != rmin) | (g["ray_max"] != rmax))[both].mean()) if both.any() else 0.0
    pass1 = ao_stats(ao1_g, ao1, gv)

    # the SD trace of the GPU's own intervals: exact
    sd_own, stats = oracle.sd_trace(osc, cam, sdp, g["depth"], g["ray_min"], g["ray_max"], r.sd_w, r.sd_h)
    assert stats[0] > 0, "no live SD rays: degenerate frame"
    sd_exact = bits_equal(g["sd"], sd_own)

    # pass 2 on the GPU's own inputs
    ao_own = oracle.svao_pass2(cam, vao, svp, g["depth"], g["normals"], g["stencil"], g["sd"], ao1_g)
    pass2 = ao_stats(g["ao"], ao_own, gv)

    report(case, frame_ao=frame, pass1_ao=pass1, pass2_ao_own_inputs=pass2, stencil_flip_frac=stencil_flip,
           touched_texel_flip_frac=touched_flip, interval_bits_differ_frac=iv_differ, sd_map_exact=sd_exact,
           live_texels=int(touched_o.sum()), stencilled_px=int((st[gv] != 0).sum()))
    assert sd_exact, (case, "SD map differs from the oracle's trace of the GPU's own intervals")
    check_ao(frame, (case, "frame"))
    check_ao(pass2, (case, "pass 2 on own inputs"))
    assert stencil_flip <= DECISION_FRAC, (case, stencil_flip)
    assert touched_flip <= DECISION_FRAC, (case, touched_flip)
    return frame


# ---- the CPU rehearsal of the sharded frames (test_sharding.py, test_band_odd.py): the oracle as the backend of
# rsd.shard.BandFrame / HaloFrame, and a free port for their gloo process groups

class OracleBackend:
    """BandFrame backend on the CPU oracle; numpy buffers shared with torch tensors."""

    def __init__(self, O, scene, cfg, ss_max_radius=None, whole_config=False):
        """whole_config: camera, VAOData and the parameter structs from every field of cfg (the odd frames), as
        tests/test_odd_geometry.py builds them; otherwise the small frames' defaults."""
        import torch
        self.O, self.cfg = O, cfg
        self.osc = O.Scene(scene.positions, scene.indices, scene.flags)
        W, H = cfg.fb_w, cfg.fb_h
        aspect = float(np.float32(W) / np.float32(H))
        N = cfg.sd_samples
        look = (scene.camera["pos"], scene.camera["target"], scene.camera["up"])
        if whole_config:
            from rsd.frame import sd_params, svao_params
            self.cam = O.camera_look_at(*look, focal_length=cfg.focal_length, frame_height=cfg.frame_height,
                                        aspect=aspect, near=cfg.near, far=cfg.far)
            self.vao, self.sd_w, self.sd_h = oracle_vao(O, W, H, cfg.divisor, cfg.sd_guard_px, cfg.radius, cfg.exponent,
                                                        cfg.thickness)
            self.sdp = to_oracle(sd_params(cfg, self.vao.sdGuard), O.SDParams)
            self.svp = to_oracle(svao_params(cfg), O.SVAOParams)
        else:
            self.cam = O.camera_look_at(*look, aspect=aspect)
            self.vao, self.sd_w, self.sd_h = oracle_vao(O, W, H, cfg.divisor, cfg.sd_guard_px, cfg.radius)
            self.sdp = O.SDParams(N, cfg.implementation, cfg.max_count, self.vao.sdGuard, 1, 1, 1, cfg.cull_mode, 0,
                                  float(np.float32(1.5 / N)))
            self.svp = O.SVAOParams(8, N, 2, 1, 1, cfg.guard_band)
        if ss_max_radius is not None:  # a small sample reach: halo windows narrower than the map
            self.vao.ssMaxRadius = ss_max_radius
        self.z, self.n = O.gbuffer(self.osc, self.cam, W, H, cfg.cull_mode, threads=2)
        self.np_ao = np.zeros((H, W), np.uint8)
        self.np_st = np.zeros((H, W), np.uint8)
        # rayMin / rayMax in one buffer, like rsd.frame.Renderer (one all-reduce per frame)
        self.np_rminmax = np.zeros((2, self.sd_h, self.sd_w), np.uint32)
        self.np_rmin, self.np_rmax = self.np_rminmax[0], self.np_rminmax[1]
        self.np_sd = np.zeros(((N + 3) // 4, self.sd_h, self.sd_w, min(N, 4)), np.float32)
        self.ao = torch.from_numpy(self.np_ao)
        self.stencil = torch.from_numpy(self.np_st)
        self.ray_minmax = torch.from_numpy(self.np_rminmax.view(np.int32))
        self.ray_min, self.ray_max = self.ray_minmax[0], self.ray_minmax[1]
        self.sd = torch.from_numpy(self.np_sd)

    def clear_intervals(self):
        self.O.svao_clear(self.np_rmin, self.np_rmax)

    def pass1(self, band=(0, 1)):
        self.O.svao_pass1_into(self.cam, self.vao, self.svp, self.z, self.n, self.np_ao, self.np_st, self.np_rmin,
                               self.np_rmax, band)

    def sd_trace(self, band=(0, 1)):
        self.O.sd_trace_into(self.osc, self.cam, self.sdp, self.z, self.np_rmin, self.np_rmax, self.np_sd, band,
                             threads=2)

    def pass2(self, band=(0, 1)):
        self.O.svao_pass2_into(self.cam, self.vao, self.svp, self.z, self.n, self.np_st, self.np_sd, self.np_ao, band,
                               threads=2)

    # contiguous bands (HaloFrame)
    def pass1_rows(self, rows):
        self.O.svao_pass1_rows_into(self.cam, self.vao, self.svp, self.z, self.n, self.np_ao, self.np_st, self.np_rmin,
                                    self.np_rmax, rows)

    def sd_trace_rows(self, rows):
        self.O.sd_trace_rows_into(self.osc, self.cam, self.sdp, self.z, self.np_rmin, self.np_rmax, self.np_sd, rows,
                                  threads=2)

    def pass2_rows(self, rows):
        self.O.svao_pass2_rows_into(self.cam, self.vao, self.svp, self.z, self.n, self.np_st, self.np_sd, self.np_ao,
                                    rows, threads=2)


def free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---- the N > 1 band frame away from the benchmark shapes (test_band_odd.py checks on the oracle and on
# HaloFrame._plan alone that the cases reach what they are meant to reach; test_gpu_band_odd.py runs
# rsd_band_frame_front / _back on them)

class BandOddCase(NamedTuple):
    frame: str       # an ODD_FRAMES name, or BAND_TALL_FRAME's
    world: int
    sd_split: str    # "tiles" or "rows"
    reach: float     # ssMaxRadius in pixels


BAND_REACH_WHOLE = 512.0   # the default ssMaxRadius: every window covers the whole of these small maps
BAND_REACH_SMALL = 24.0    # SVAO_SWEEP's clamping value: windows of a few dozen rows

# A window that neither map edge clips needs more rows than any ODD_FRAMES shape has: at a reach of 24 px the sample
# reach is 40 to 60 rows of the frame buffer either way (rsd.shard.halo_px), the tallest odd frame has 103.  This one
# is tall and narrow instead: 37 x 203 visible (7 groups, the last of 11 rows), guard 3, divisor 2, sdGuard 5 / 2 = 2,
# SD map 26 x 109
BAND_TALL_FRAME = OddFrame("tall_div2", 37, 203, 3, 2, 5, 2.0)


def band_frame_shape(name):
    return BAND_TALL_FRAME if name == BAND_TALL_FRAME.name else odd_frame(name)


def band_odd_worlds(f):
    """2, 3, 5 and one more than the frame has 32-row groups (at least one rank without a row)."""
    return sorted({2, 3, 5, -(-f.visible_h // 32) + 1})


def _band_odd_cases():
    # one (split, reach) per (frame, world), dealt in turn so that each reach meets each split on every frame with
    # four worlds and over the table in any case
    kinds = [("tiles", BAND_REACH_WHOLE), ("rows", BAND_REACH_SMALL), ("rows", BAND_REACH_WHOLE),
             ("tiles", BAND_REACH_SMALL)]
    cases, i = [], 0
    for f in ODD_FRAMES:
        for world in band_odd_worlds(f):
            cases.append(BandOddCase(f.name, world, *kinds[i % 4]))
            i += 1
    # the tall frame at the small reach only (its whole-map windows add nothing to the odd frames')
    cases += [BandOddCase(BAND_TALL_FRAME.name, 3, "tiles", BAND_REACH_SMALL),
              BandOddCase(BAND_TALL_FRAME.name, 5, "rows", BAND_REACH_SMALL)]
    return cases


BAND_ODD_CASES = _band_odd_cases()


def band_case_id(c):
    return f"{c.frame}_w{c.world}_{c.sd_split}_r{c.reach:g}"


class NoComm:
    """The communicator of a HaloFrame that only plans (no frame is run)."""
    nccl = False


def band_plans(backend, world, sd_split):
    """HaloFrame's partition of `backend`'s frame as every rank of `world` sees it (nothing is exchanged)."""
    from rsd.shard import HaloFrame
    return [HaloFrame(backend, r, world, comm=NoComm(), rebalance=False, sd_split=sd_split) for r in range(world)]


def band_region_rows(plan, region):
    """The SD rows of a send / receive region of a plan (None: no rows)."""
    if not region:
        return []
    return plan._region_rows(region[0], region[1], plan.world if plan.sd_split == "tiles" else 1)


def band_touched(backend, rows):
    """The SD texels that pass 1 of the visible rows `rows` touches on cleared interval maps (rayMin no longer
    asuint(FLT_MAX), or rayMax no longer 0), on the oracle."""
    O = backend.O
    rmin, rmax = np.zeros_like(backend.np_rmin), np.zeros_like(backend.np_rmax)
    O.svao_clear(rmin, rmax)
    ao, st = np.zeros_like(backend.np_ao), np.zeros_like(backend.np_st)
    O.svao_pass1_rows_into(backend.cam, backend.vao, backend.svp, backend.z, backend.n, ao, st, rmin, rmax, rows)
    return (rmin != 0x7F7FFFFF) | (rmax != 0)


def band_odd_backend(O, c, scene=None):
    """The oracle backend of a BAND_ODD_CASES entry over arcade_tiny."""
    from rsd.scenes import make_scene
    return OracleBackend(O, scene or make_scene("arcade_tiny"), odd_frame_config(band_frame_shape(c.frame)), c.reach,
                         whole_config=True)


# ---- the band frame over moving scenes (test_band_odd.py: the steps differ; test_gpu_band_odd.py: the frames)

def moved_positions(scene, seed, part=(0.4, 0.3, -0.5)):
    """Per-vertex jitter of a fixed seed plus the last eighth of the triangles translated by `part`."""
    rng = np.random.default_rng(seed)
    p = scene.positions + (0.02 * rng.standard_normal(scene.positions.shape)).astype(np.float32)
    v = np.unique(scene.indices[-max(1, scene.indices.shape[0] // 8):])
    p[v] += np.float32(part)
    return np.ascontiguousarray(p, np.float32)


BAND_MOVING_WORLD = 3
# 1.9 is past the last keyframe (1.5): both animations cycle.  (From rest, t = 0.37 moves 86 SD texels of the oracle's
# map at band_moving_config(), below the 100 that test_band_odd.py asks of neighbouring steps; these move 116 to 138.)
TURNSTILE_TIMES = (0.6, 1.1, 1.9)


def band_moving_config():
    """SVAO_RAGGED_VISIBLE: 200 x 120 visible, guard 16, divisor 2, N = 4."""
    return small_frame_config(visible=SVAO_RAGGED_VISIBLE, guard=16, divisor=2, N=4)


def band_dynamic_steps(scene):
    """The positions of the dynamic sequence: P0, P1 (update_positions), P2 (update_subset of the vertices in which
    P1 and P2 differ), P0 again -- as (name, positions); the subset's ids are band_subset_ids(P1, P2)."""
    p0 = np.ascontiguousarray(scene.positions, np.float32)
    return [("P0", p0), ("P1", moved_positions(scene, 1)), ("P2", moved_positions(scene, 2)), ("P0 again", p0)]


def band_subset_ids(a, b):
    return np.flatnonzero((a != b).any(axis=1)).astype(np.uint32)


def turnstile_steps():
    """The built turnstile scene (with its rig) and its positions at rest and at TURNSTILE_TIMES, posed by
    tests/skinning_checker.py -- as (scene, [(name, positions)])."""
    from pathlib import Path

    import skinning_checker
    from rsd.pyscene import load_pyscene
    scene = load_pyscene(Path(__file__).resolve().parent / "fixtures" / "turnstile.pyscene").build("turnstile")
    assert scene.rig is not None
    steps = [("rest", np.ascontiguousarray(scene.positions, np.float32))]
    steps += [(f"t = {t:g}", skinning_checker.posed(scene.positions, scene.rig, scene.rig.matrices(t)))
              for t in TURNSTILE_TIMES]
    return scene, steps
