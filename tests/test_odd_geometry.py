"""The frames of odd geometry reach the branches they are meant to reach (CPU: the oracle, and librsd's host code).

tests/test_gpu_odd_geometry.py runs the G-buffer, both SVAO passes and the SD trace on helpers.ODD_FRAMES: visible
sizes that are no multiple of 8, odd guard bands, divisor 3, SD guards that the divisor does not divide, a frame
smaller than one workgroup, a frame one pixel over a multiple of 32.  A green parity test there means nothing if the
frame requests no SD rays or its SD map happens to be a multiple of the 8 x 8 tile, so this module checks the inputs
on the oracle alone, as tests/test_svao_params.py does for the parameter sweep:

  * SD map size: for every shape but `tiny` neither dimension is a multiple of 8; for `tiny` both are below 32;
  * enough work: every shape but `tiny` has a non-zero pass-1 stencil on at least 1000 visible pixels and an
    interval (ray_max != 0) on at least 300 SD texels; `tiny` at least 50 stencilled pixels in the whole buffer and
    30 touched texels;
  * guard-band stores: every shape with a guard band has at least 50 stencilled pixels inside the right or bottom
    guard band -- pass 1's padded dispatch writes past the visible region, as the reference's compute dispatch of
    roundup32(visible) threads does (SVAO.cpp:347-350);
  * the SD trace did work: at least 100 texels (`tiny`: 10) of the oracle's SD map differ from the cleared value.

These are conditions on the inputs, not measurements: a shape that misses one is replaced, the condition stays.

librsd's host code is checked here as well: rsd_svao_make_vao_data gives the SD map size and the VAOData that
SVAO::compile gives (helpers.oracle_vao: lowResolution = ceil(fb / divisor), sdGuard = sd_guard_px / divisor as an
integer division), at every shape."""
import ctypes as C

import numpy as np
import pytest

from helpers import (ODD_FRAMES, ODD_SD_SIZES, odd_frame_config, odd_second_pose, oracle_vao, right_bottom_guard,
                     to_oracle, visible_region)

DEFAULT_DEPTH = np.float32(1.0)  # the cleared SD texel of a normalised map (StochasticDepthMapRT: Normalize)

_IDS = [f.name for f in ODD_FRAMES]
_frames = {}


def _frame(O, f, second_pose=False):
    """The oracle's G-buffer, pass 1 and SD trace of arcade_tiny on the shape f, from the scene's own camera or from
    helpers.odd_second_pose (computed once)."""
    if (f.name, second_pose) not in _frames:
        from rsd.frame import sd_params, svao_params
        from rsd.scenes import make_scene
        cfg = odd_frame_config(f)
        W, H = cfg.fb_w, cfg.fb_h
        s = make_scene("arcade_tiny")
        pos, target, up = odd_second_pose(s) if second_pose else (s.camera["pos"], s.camera["target"], s.camera["up"])
        cam = O.camera_look_at(pos, target, up, focal_length=cfg.focal_length,
                               frame_height=cfg.frame_height, aspect=float(np.float32(W) / np.float32(H)),
                               near=cfg.near, far=cfg.far)
        osc = O.Scene(s.positions, s.indices, s.flags)
        z, n = O.gbuffer(osc, cam, W, H, cfg.cull_mode)
        vao, sd_w, sd_h = oracle_vao(O, W, H, cfg.divisor, cfg.sd_guard_px, cfg.radius, cfg.exponent, cfg.thickness)
        svp = to_oracle(svao_params(cfg), O.SVAOParams)
        ao1, st, rmin, rmax = O.svao_pass1(cam, vao, svp, z, n, sd_w, sd_h)
        sdp = to_oracle(sd_params(cfg, vao.sdGuard), O.SDParams)
        sd, stats = O.sd_trace(osc, cam, sdp, z, rmin, rmax, sd_w, sd_h)
        _frames[f.name, second_pose] = dict(cfg=cfg, vao=vao, sd_w=sd_w, sd_h=sd_h, stencil=st, ray_max=rmax, sd=sd,
                                            stats=stats)
    return _frames[f.name, second_pose]


def test_shapes_are_the_odd_ones():
    """The shapes themselves: no visible size is a multiple of 8, `one_over` is one pixel over a multiple of 32 in
    both axes with guard 1 and divisor 1, `tiny` is smaller than one 32 x 32 workgroup, `no_guards` has neither guard
    (sdGuard 0 selects the generic pass 1), a divisor of 3 and an SD guard that its divisor does not divide occur."""
    by = {f.name: f for f in ODD_FRAMES}
    assert set(by) == set(ODD_SD_SIZES) and len(by) == len(ODD_FRAMES) == 5
    for f in ODD_FRAMES:
        assert f.visible_w % 8 and f.visible_h % 8, f
    o = by["one_over"]
    assert o.visible_w % 32 == 1 and o.visible_h % 32 == 1 and (o.guard, o.divisor) == (1, 1)
    assert by["tiny"].visible_w < 32 and by["tiny"].visible_h < 32
    assert (by["no_guards"].guard, by["no_guards"].sd_guard_px) == (0, 0)
    assert by["odd_div3"].divisor == 3
    assert any(f.sd_guard_px % f.divisor for f in ODD_FRAMES)
    assert {f.divisor for f in ODD_FRAMES} >= {1, 2, 3, 4}


@pytest.mark.parametrize("f", ODD_FRAMES, ids=_IDS)
def test_librsd_sd_map_size_is_svao_compiles(oracle, f):
    """rsd_svao_make_vao_data against SVAO::compile restated in helpers.oracle_vao, and against the sizes written
    down beside the shapes: the low resolution rounds up, the SD guard rounds down."""
    from rsd import abi
    from rsd.frame import make_vao
    cfg = odd_frame_config(f)
    vao, sd_w, sd_h = make_vao(cfg)
    want, ow, oh = oracle_vao(oracle, cfg.fb_w, cfg.fb_h, cfg.divisor, cfg.sd_guard_px, cfg.radius, cfg.exponent,
                              cfg.thickness)
    assert (sd_w, sd_h) == (ow, oh) == ODD_SD_SIZES[f.name]
    assert C.sizeof(abi.VAOData) == C.sizeof(oracle.VAOData)
    assert bytes(vao) == bytes(want)
    assert vao.sdGuard == f.sd_guard_px // f.divisor
    assert tuple(vao.lowResolution) == (-(-cfg.fb_w // f.divisor), -(-cfg.fb_h // f.divisor))


@pytest.mark.parametrize("f", ODD_FRAMES, ids=_IDS)
def test_shape_reaches_its_branches(oracle, f):
    o = _frame(oracle, f)
    cfg = o["cfg"]
    sd_w, sd_h = o["sd_w"], o["sd_h"]
    assert (sd_w, sd_h) == ODD_SD_SIZES[f.name]
    st = o["stencil"] != 0
    stencilled, visible = int(st.sum()), int(st[visible_region(cfg)].sum())
    in_guard = int(st[right_bottom_guard(cfg)].sum())
    touched = int((o["ray_max"] != 0).sum())
    traced = int((o["sd"] != DEFAULT_DEPTH).any(axis=(0, 3)).sum())
    print(f"{f.name}: SD map {sd_w} x {sd_h}; stencilled {stencilled} px ({visible} visible, {in_guard} in the right / "
          f"bottom guard band), touched {touched} SD texels, {traced} texels off the cleared value, "
          f"{int(o['stats'][0])} live rays")
    if f.name == "tiny":
        assert sd_w < 32 and sd_h < 32
        assert stencilled >= 50
        assert touched >= 30
        assert traced >= 10
    else:
        assert sd_w % 8 and sd_h % 8
        assert visible >= 1000
        assert touched >= 300
        assert traced >= 100
    if f.guard:
        assert in_guard >= 50
    else:
        assert in_guard == 0


@pytest.mark.parametrize("f", ODD_FRAMES, ids=_IDS)
def test_second_pose_touches_other_texels(oracle, f):
    """The clean-tile test renders two poses: texels touched from the first and not from the second (the trace of the
    second frame has to put them back to the cleared value) and the other way round, at least 10 texels each way
    (`tiny`: 1 -- most of its 57 touched texels belong to the forced rays of samples outside the screen, which the
    frame's geometry places, not the pose).  (The 8 x 8 tiles that change between live and clean are printed: on these small maps few tiles are
    ever clean, the large clean regions are test_gpu_clean_tiles.py's.)"""
    a, b = _frame(oracle, f)["ray_max"] != 0, _frame(oracle, f, second_pose=True)["ray_max"] != 0
    h, w = a.shape

    def tiles(m):
        p = np.zeros(((h + 7) // 8 * 8, (w + 7) // 8 * 8), bool)
        p[:h, :w] = m
        return p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).any(axis=(1, 3))

    gone, new = int((a & ~b).sum()), int((b & ~a).sum())
    ta, tb = tiles(a), tiles(b)
    print(f"{f.name}: {gone} texels touched only from the first pose, {new} only from the second; tiles "
          f"{int((ta & ~tb).sum())} / {int((tb & ~ta).sum())}")
    need = 1 if f.name == "tiny" else 10
    assert gone >= need and new >= need
