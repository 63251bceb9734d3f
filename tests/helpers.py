"""Shared test helpers: struct conversion between librsd and the oracle, the oracle side of a whole
frame (G-buffer -> pass 1 -> SD trace -> pass 2), the SVAO parameter sweep of test_svao_params.py /
test_gpu_svao_params.py, the frames of odd geometry of test_odd_geometry.py / test_gpu_odd_geometry.py, and the
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
