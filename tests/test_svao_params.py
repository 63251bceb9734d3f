"""The SVAO parameter sweep reaches the branches it is meant to reach (CPU oracle only).

tests/test_gpu_svao_params.py runs the SVAO kernels away from the default parameter point
(exponent 2, thickness 0, ssRadiusCutoff 6, ssMaxRadius 512): a clamped screen radius, exponent != 2,
thickness != 0.  A green parity test there means nothing if its frame never takes those branches, so this
module checks the inputs on the oracle alone, at every point and frame the GPU module uses (both import
the points from helpers.SVAO_SWEEP):

  * a clamped point (helpers.SVAO_CLAMPED_POINTS): at least 1000 visible pixels with radiusInPixels >
    ssMaxRadius and at least 1000 without -- radiusInPixels recomputed from the depth in numpy float32
    with BasicAOData::Init's formula (Common.slang:296-303);
  * every point: at least 300 visible pixels with a non-zero stencil and at least 300 SD texels with an
    interval (ray_max != 0);
  * every non-default exponent / thickness: the pass-1 AO differs from the pass-1 AO at exponent 2,
    thickness 0 (every other parameter as at the point) on at least 1000 visible pixels.

These are conditions on the inputs, not measurements: a point that misses one is replaced, the condition
stays."""
import numpy as np
import pytest

from helpers import (SVAO_CLAMPED_POINTS, SVAO_DEFAULT_POINT, SVAO_RAGGED_VISIBLE, SVAO_SMALL_VISIBLE, SVAO_SWEEP,
                     oracle_vao, radius_in_pixels, set_svao_point, svao_point_config, svao_point_id, visible_region)

MIN_CLAMPED = 1000    # visible pixels on either side of the ssMaxRadius clamp
MIN_STENCILLED = 300  # visible pixels with a non-zero stencil
MIN_TOUCHED = 300     # SD texels with an interval
MIN_CHANGED = 1000    # visible pixels whose pass-1 AO a non-default exponent / thickness changes
MIN_MODE = 100        # stencilled pixels / touched texels of a mode case (test_mode_cases_request_rays)

_gbuffers = {}


def _pass1(O, point, visible=SVAO_SMALL_VISIBLE, nd=8, kernel=0):
    """The oracle's G-buffer (one per frame size, shared) and pass 1 of arcade_tiny at `point`."""
    from rsd.scenes import make_scene
    cfg = svao_point_config(point, visible=visible)
    W, H = cfg.fb_w, cfg.fb_h
    if (W, H) not in _gbuffers:
        s = make_scene("arcade_tiny")
        cam = O.camera_look_at(s.camera["pos"], s.camera["target"], s.camera["up"], focal_length=cfg.focal_length,
                               frame_height=cfg.frame_height, aspect=float(np.float32(W) / np.float32(H)),
                               near=cfg.near, far=cfg.far)
        z, n = O.gbuffer(O.Scene(s.positions, s.indices, s.flags), cam, W, H, cfg.cull_mode)
        z.setflags(write=False)
        n.setflags(write=False)
        _gbuffers[W, H] = cam, z, n
    cam, z, n = _gbuffers[W, H]
    vao, sd_w, sd_h = oracle_vao(O, W, H, cfg.divisor, cfg.sd_guard_px, cfg.radius, cfg.exponent, cfg.thickness)
    set_svao_point(vao, point)
    svp = O.SVAOParams(nd, cfg.sd_samples, 2, 1, 1, cfg.guard_band, 0, None, 0, kernel)
    ao1, st, rmin, rmax = O.svao_pass1(cam, vao, svp, z, n, sd_w, sd_h)
    return dict(cfg=cfg, cam=cam, vao=vao, depth=z, ao1=ao1, stencil=st, ray_max=rmax, gv=visible_region(cfg))


def test_sweep_is_away_from_the_default_point():
    """Every sweep point differs from the default in exponent or thickness or clamps the radius, the
    clamped points are sweep points, and the points are distinct VAOData (the constant cache's keys)."""
    assert len(set(SVAO_SWEEP + [SVAO_DEFAULT_POINT])) == len(SVAO_SWEEP) + 1
    for i, p in enumerate(SVAO_SWEEP):
        assert p[:2] != SVAO_DEFAULT_POINT[:2] or i in SVAO_CLAMPED_POINTS, p
    for i in SVAO_CLAMPED_POINTS:
        assert SVAO_SWEEP[i][2] < SVAO_DEFAULT_POINT[2]


def test_radius_formula_is_the_oracles(oracle):
    """The numpy radiusInPixels is the oracle's, checked through the one place the oracle shows it:
    radiusInPixels < 0.5 makes BasicAOData::Init fail (Common.slang:305), AO = 1 and stencil 0.  With the
    AO radius chosen so that the median pixel sits at that threshold, every pixel the formula puts below
    it gets AO = 1 and no stencil from the oracle, and the oracle computes an AO for the others."""
    o = _pass1(oracle, SVAO_DEFAULT_POINT)
    rip = radius_in_pixels(o["cam"], o["vao"], o["depth"])[o["gv"]]
    # scale the radius so that the frame's median pixel sits exactly at the 0.5-px threshold
    med = float(np.median(rip))
    point = SVAO_DEFAULT_POINT[:4] + (float(np.float32(0.5 / med)),)
    o = _pass1(oracle, point)
    rip = radius_in_pixels(o["cam"], o["vao"], o["depth"])[o["gv"]]
    below = rip < np.float32(0.5)
    assert 1000 < below.sum() < below.size - 1000
    ao, st = o["ao1"][o["gv"]], o["stencil"][o["gv"]]
    assert (ao[below] == 255).all() and (st[below] == 0).all()
    assert (ao[~below] != 255).sum() > 1000  # ... and computes an AO for above it


@pytest.mark.parametrize("index,visible", [(i, SVAO_SMALL_VISIBLE) for i in range(len(SVAO_SWEEP))] +
                         [(1, SVAO_RAGGED_VISIBLE)],
                         ids=lambda v: svao_point_id(SVAO_SWEEP[v]) if isinstance(v, int) else "x".join(map(str, v)))
def test_sweep_point_reaches_its_branches(oracle, index, visible):
    point = SVAO_SWEEP[index]
    o = _pass1(oracle, point, visible)
    gv = o["gv"]
    rip = radius_in_pixels(o["cam"], o["vao"], o["depth"])[gv]
    clamped = rip > np.float32(point[2])
    stencilled = int((o["stencil"][gv] != 0).sum())
    touched = int((o["ray_max"] != 0).sum())
    print(f"{svao_point_id(point)} {visible}: clamped {int(clamped.sum())} of {clamped.size} px, "
          f"stencilled {stencilled} px, touched {touched} SD texels")
    if index in SVAO_CLAMPED_POINTS:
        assert clamped.sum() >= MIN_CLAMPED, "too few clamped pixels"
        assert (~clamped).sum() >= MIN_CLAMPED, "too few unclamped pixels"
    elif point[2] >= SVAO_DEFAULT_POINT[2]:
        assert not clamped.any()
    assert stencilled >= MIN_STENCILLED
    assert touched >= MIN_TOUCHED
    if point[:2] != SVAO_DEFAULT_POINT[:2]:
        base = _pass1(oracle, SVAO_DEFAULT_POINT[:2] + point[2:], visible)
        changed = int((o["ao1"][gv] != base["ao1"][gv]).sum())
        print(f"  pass-1 AO differs from exponent 2 / thickness 0 on {changed} px")
        assert changed >= MIN_CHANGED
        # ... and each of the two parameters alone
        for k in (0, 1):
            if point[k] != SVAO_DEFAULT_POINT[k]:
                alone = list(SVAO_DEFAULT_POINT[:2]) + list(point[2:])
                alone[k] = point[k]
                one = _pass1(oracle, tuple(alone), visible)
                n = int((one["ao1"][gv] != base["ao1"][gv]).sum())
                print(f"  {('exponent', 'thickness')[k]} alone: {n} px")
                assert n >= MIN_CHANGED


@pytest.mark.parametrize("index,nd,kernel", [(1, 8, 1), (2, 8, 1), (2, 16, 0)],
                         ids=["hbao_point2", "hbao_point3", "vao16_point3"])
def test_mode_cases_request_rays(oracle, index, nd, kernel):
    """The HBAO and 16-direction cases of the GPU module at their sweep points request SD rays as well.  The
    bounds of the sweep itself are for the VAO kernel; HBAO's requireRay is the stricter test (Common.slang:
    455-461), so here the bound is MIN_MODE: more pixels and texels than one 64-lane wave holds, so that the
    refined branch runs in several waves and tiles."""
    o = _pass1(oracle, SVAO_SWEEP[index], nd=nd, kernel=kernel)
    stencilled, touched = int((o["stencil"][o["gv"]] != 0).sum()), int((o["ray_max"] != 0).sum())
    print(f"{svao_point_id(SVAO_SWEEP[index])} nd {nd} kernel {kernel}: stencilled {stencilled} px, touched {touched}")
    assert stencilled >= MIN_MODE
    assert touched >= MIN_MODE
