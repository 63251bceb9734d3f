"""The SVAO kernels away from their default parameter point, against the oracle.

Every other GPU test of the SVAO passes runs at exponent 2, thickness 0, ssRadiusCutoff 6, ssMaxRadius 512
and a depth range inside the fast-division window.  The kernels carry branches taken only away from it:

  * a screen radius clamped to ssMaxRadius (svao_math.h basic_init shrinks the pixel's AO radius;
    sample_init then leaves the host-evaluated direction terms: exact numerics compute the sqrt per
    direction, fast numerics rescale the host terms in the SCALED loop);
  * exponent != 2 (rsd_device.h acc_pow: the device's double pow instead of x * x);
  * thickness != 0 (constRadius, the halo term, requireRay, the Raytraced mode's tHalo0 / tCRS);
  * the generic pass-1 / pass-2 kernels on a frame the specialised ones would take (RSD_PASS1 /
    RSD_PASS2 = generic);
  * svao.hip cached_consts evicting and refilling its four entries;
  * depths outside [pzLo, pzHi] in exact numerics (the div_unscaled_*_ok guards and the wave-level
    __ballot fallbacks).

The points are helpers.SVAO_SWEEP; tests/test_svao_params.py checks on the oracle alone that each of them
reaches its branches (enough clamped / unclamped / stencilled pixels and touched SD texels, and an
exponent / thickness that changes the AO).  Exact numerics are bit-identical to the oracle; fast numerics
are graded by BASELINE.md section 4's tolerance (helpers.grade), also on the clamped and on the unclamped
pixels alone.  RSD_NUMERICS_REPORT=<path> collects the measured figures."""

import numpy as np
import pytest

from helpers import (SVAO_CLAMPED_POINTS, SVAO_DEFAULT_POINT, SVAO_RAGGED_VISIBLE, SVAO_SMALL_VISIBLE, SVAO_SWEEP,
                     ao_stats, bits_equal, check_ao, grade, radius_in_pixels, report, set_svao_point, svao_point_config,
                     svao_point_id, to_oracle, visible_region)

pytestmark = pytest.mark.gpu

MIN_CLAMPED = 1000  # clamped visible pixels of a clamped point (test_svao_params.py checks it on the oracle)


def _structs(r, O):
    return (to_oracle(r.cam, O.Camera), to_oracle(r.vao, O.VAOData), to_oracle(r.sdp, O.SDParams),
            to_oracle(r.svp, O.SVAOParams))


def _renderer(point, numerics="exact", visible=SVAO_SMALL_VISIBLE, divisor=2, gpu_scene=None, dev=None, **kw):
    """A renderer of arcade_tiny at a sweep point: exponent, thickness and radius through the FrameConfig,
    ssMaxRadius and ssRadiusCutoff written into its VAOData (to_oracle copies the struct to the oracle)."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rsd.frame import Renderer
    from rsd.scenes import make_scene
    scene = make_scene("arcade_tiny")
    r = Renderer(scene, svao_point_config(point, visible=visible, divisor=divisor, numerics=numerics, **kw),
                 gpu_scene=gpu_scene, dev=dev)
    assert (r.vao.exponent, r.vao.thickness, r.vao.radius) == (point[0], point[1], point[4])
    set_svao_point(r.vao, point)
    return r, scene


def _second_layer(depth):
    """A second depth layer behind the first (DualDepth primary), as test_gpu_kernels.py builds it."""
    return depth * np.float32(1.1) + np.float32(0.25)


def _oracle_frame(O, r, scene, g1, depth2=None):
    """The oracle's frame on the GPU's G-buffer g1 with r's structs: pass 1, SD trace / Raytraced, pass 2."""
    cfg = r.cfg
    cam, vao, sdp, svp = _structs(r, O)
    osc = O.Scene(scene.positions, scene.indices, scene.flags)
    ao1, st, rmin, rmax = O.svao_pass1(cam, vao, svp, g1["depth"], g1["normals"], r.sd_w, r.sd_h, depth2=depth2)
    o = dict(ao1=ao1, stencil=st, ray_min=rmin, ray_max=rmax)
    if cfg.secondary == 2:
        o["sd"], _ = O.sd_trace(osc, cam, sdp, g1["depth"], rmin, rmax, r.sd_w, r.sd_h)
        o["ao"] = O.svao_pass2(cam, vao, svp, g1["depth"], g1["normals"], st, o["sd"], ao1, depth2=depth2)
    else:
        o["ao"] = O.svao_pass2_raytraced(osc, cam, vao, svp, g1["depth"], g1["normals"], st, ao1, cull=cfg.cull_mode,
                                         ray_pipeline=int(cfg.ray_pipeline), depth2=depth2)
    return o


def _gpu_frame(r):
    """test_gpu_kernels.py's _frame: clear, pass 1, snapshot, the whole frame, snapshot."""
    r.clear_intervals()
    r.pass1()
    g1 = r.numpy()
    r.frame()
    return g1, r.numpy()


def _assert_exact(r, g1, g, o, what):
    gv = visible_region(r.cfg)
    assert np.array_equal(g1["stencil"], o["stencil"]), (what, "stencil")
    assert np.array_equal(g1["ao"], o["ao1"]), (what, "pass-1 AO")
    if r.cfg.secondary == 2:
        assert np.array_equal(g1["ray_min"], o["ray_min"]) and np.array_equal(g1["ray_max"], o["ray_max"]), \
            (what, "intervals")
        if "sd" in o:
            assert bits_equal(g["sd"], o["sd"]), (what, "SD map")
        assert np.array_equal(g["ao"][gv], o["ao"][gv]), (what, "frame AO")
    else:
        assert np.array_equal(g["ao"], o["ao"]), (what, "Raytraced frame AO")


# ---- a. exact parity over the sweep

# (sweep point, AO kernel, primary, secondary, directions, dualAO, visible): VAO / StochasticDepth at every
# point; HBAO at the second and third; DualDepth primary at the second; 16 directions with dualAO at the
# third; the Raytraced secondary mode (divisor 1; thickness enters svao_rt.hip) at the first and second
# with both kernels; a ragged visible size at the second
_PARITY = ([(i, "vao", 0, 2, 8, False, SVAO_SMALL_VISIBLE) for i in range(len(SVAO_SWEEP))] +
           [(1, "hbao", 0, 2, 8, False, SVAO_SMALL_VISIBLE), (2, "hbao", 0, 2, 8, False, SVAO_SMALL_VISIBLE),
            (1, "vao", 1, 2, 8, False, SVAO_SMALL_VISIBLE),
            (2, "vao", 0, 2, 16, True, SVAO_SMALL_VISIBLE),
            (0, "vao", 0, 3, 8, False, SVAO_SMALL_VISIBLE), (0, "hbao", 0, 3, 8, False, SVAO_SMALL_VISIBLE),
            (1, "vao", 0, 3, 8, False, SVAO_SMALL_VISIBLE), (1, "hbao", 0, 3, 8, False, SVAO_SMALL_VISIBLE),
            (1, "vao", 0, 2, 8, False, SVAO_RAGGED_VISIBLE)])


def _parity_id(c):
    i, kernel, primary, secondary, nd, dual, visible = c
    return "-".join([f"p{i + 1}", kernel, ("single", "dual")[primary], {2: "sd", 3: "rt"}[secondary], f"d{nd}"] +
                    (["dualao"] if dual else []) + (["ragged"] if visible != SVAO_SMALL_VISIBLE else []))


@pytest.mark.parametrize("case", _PARITY, ids=_parity_id)
def test_sweep_exact_parity(oracle, case):
    """Stencil, intervals and pass-1 AO bit-equal to oracle.svao_pass1, the SD map to oracle.sd_trace, the
    frame AO to oracle.svao_pass2 / svao_pass2_raytraced, at a sweep point."""
    i, kernel, primary, secondary, nd, dual, visible = case
    r, scene = _renderer(SVAO_SWEEP[i], visible=visible, divisor=1 if secondary == 3 else 2, ao_kernel=kernel,
                         primary=primary, secondary=secondary, num_directions=nd, dual_ao=dual)
    r.gbuffer()
    if primary == 1:
        r.depth2.copy_(r.depth * 1.1 + 0.25)
    g1, g = _gpu_frame(r)
    d2 = _second_layer(g1["depth"]) if primary == 1 else None
    if d2 is not None:
        assert bits_equal(r.depth2.cpu().numpy(), d2)
    o = _oracle_frame(oracle, r, scene, g1, d2)
    assert (o["stencil"] != 0).sum() > 50, "no refined directions: the test frame is degenerate"
    _assert_exact(r, g1, g, o, _parity_id(case))
    assert not np.array_equal(g["ao"], g1["ao"]), "pass 2 changed nothing"
    r.close()


# ---- b. the specialised and the generic kernels agree

# RSD_PASS1 / RSD_PASS2 (read by librsd on every call): unset, both generic, and one of each
_KERNEL_CHOICES = [(None, None), ("generic", "generic"), ("generic", None), (None, "generic")]
_SPEC_POINTS = [SVAO_DEFAULT_POINT, SVAO_SWEEP[1], SVAO_SWEEP[3]]


def _with_kernels(monkeypatch, p1, p2):
    for name, v in (("RSD_PASS1", p1), ("RSD_PASS2", p2)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


@pytest.mark.parametrize("point", _SPEC_POINTS, ids=svao_point_id)
def test_specialised_and_generic_kernels_agree_exact(oracle, monkeypatch, point):
    """The same pass 1 and pass 2 through the specialised kernels, the generic ones, and one of each:
    stencil, intervals, pass-1 AO, SD map and frame AO bit-identical across the runs and to the oracle."""
    r, scene = _renderer(point)
    r.gbuffer()
    runs = []
    for p1, p2 in _KERNEL_CHOICES:
        _with_kernels(monkeypatch, p1, p2)
        r.ao.zero_()
        r.stencil.zero_()
        runs.append(_gpu_frame(r))
    o = _oracle_frame(oracle, r, scene, runs[0][0])
    for (g1, g), choice in zip(runs, _KERNEL_CHOICES):
        _assert_exact(r, g1, g, o, (svao_point_id(point), choice))
        for k in ("stencil", "ray_min", "ray_max", "ao"):
            assert np.array_equal(g1[k], runs[0][0][k]), (choice, "pass 1", k)
        assert np.array_equal(g["ao"], runs[0][1]["ao"]) and bits_equal(g["sd"], runs[0][1]["sd"]), (choice, "frame")
    r.close()


@pytest.mark.parametrize("point", _SPEC_POINTS, ids=svao_point_id)
def test_specialised_and_generic_kernels_agree_fast(oracle, monkeypatch, point):
    """Fast numerics: each kernel choice within the AO tolerance of the oracle's exact frame; the
    specialised-versus-generic difference is reported, not bounded."""
    r, scene = _renderer(point, numerics="fast")
    r.gbuffer()
    runs = []
    for p1, p2 in _KERNEL_CHOICES:
        _with_kernels(monkeypatch, p1, p2)
        r.ao.zero_()
        r.stencil.zero_()
        runs.append(_gpu_frame(r))
    o = _oracle_frame(oracle, r, scene, runs[0][0])
    gv = visible_region(r.cfg)
    spec = runs[0][1]
    for (g1, g), choice in zip(runs, _KERNEL_CHOICES):
        s = ao_stats(g["ao"], o["ao"], gv)
        d = ao_stats(g["ao"], spec["ao"], gv)
        report(f"spec_vs_generic_{svao_point_id(point)}", pass1=choice[0] or "specialised",
               pass2=choice[1] or "specialised", frame_ao=s, vs_specialised=d,
               stencil_differs_px=int((g["stencil"][gv] != spec["stencil"][gv]).sum()))
        print(svao_point_id(point), choice, "vs oracle", s, "vs specialised", d)
        check_ao(s, (svao_point_id(point), choice))
    r.close()


# ---- c. fast numerics on the clamped pixels alone

@pytest.mark.parametrize("index", [1, 3, 0], ids=lambda i: svao_point_id(SVAO_SWEEP[i]))
def test_fast_numerics_clamped_subset(oracle, index):
    """helpers.grade's checks of the whole frame, and the same AO tolerance on the clamped visible pixels
    alone and on the unclamped ones alone: the whole-frame statistics would absorb an error of the SCALED
    rescaling confined to the few percent of pixels nearest the camera.  (The first sweep point clamps
    nothing: fast numerics with exponent != 2 and thickness != 0.)"""
    point = SVAO_SWEEP[index]
    r, scene = _renderer(point, numerics="fast")
    r.gbuffer()
    detail = {}
    case = f"sweep_{svao_point_id(point)}"
    grade(oracle, r, scene, case, detail)
    g, ao, gv = detail["gpu"], detail["ao"], detail["gv"]
    clamped = radius_in_pixels(r.cam, r.vao, g["depth"])[gv] > np.float32(point[2])
    subsets = {}
    if index in SVAO_CLAMPED_POINTS:
        assert clamped.sum() >= MIN_CLAMPED and (~clamped).sum() >= MIN_CLAMPED, int(clamped.sum())
        subsets["clamped"] = ao_stats(g["ao"], ao, gv, clamped)
    else:
        assert not clamped.any()
    subsets["unclamped"] = ao_stats(g["ao"], ao, gv, ~clamped)
    report(case + "_subsets", clamped_px=int(clamped.sum()), unclamped_px=int((~clamped).sum()), **subsets)
    print(case, "clamped px", int(clamped.sum()), subsets)
    for name, s in subsets.items():
        check_ao(s, (case, name))
    r.close()


# ---- d. the constant cache (svao.hip cached_consts: four thread-local entries, replaced in turn)

def _pass1_snapshot(r):
    r.ao.zero_()
    r.stencil.zero_()
    r.clear_intervals()
    r.pass1()
    g = r.numpy()
    return {k: g[k] for k in ("stencil", "ray_min", "ray_max", "ao")}


def _assert_pass1(a, b, what):
    for k in ("stencil", "ray_min", "ray_max"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert np.array_equal(a["ao"], b["ao1"] if "ao1" in b else b["ao"]), (what, "pass-1 AO")


def test_constant_cache_eviction_vao_data(oracle):
    """Six distinct VAOData in one process (the five sweep points and the default) evict and refill the
    four cache entries; then the first again (a refill of an evicted entry), the second-to-last (a hit) and
    the third (evicted by that refill): every run equals the oracle's pass 1 and its own first run."""
    points = SVAO_SWEEP + [SVAO_DEFAULT_POINT]
    r, scene = _renderer(points[0])
    r.gbuffer()
    depth, normals = r.numpy()["depth"], r.numpy()["normals"]
    first, ref = [], []
    for p in points:
        set_svao_point(r.vao, p)
        first.append(_pass1_snapshot(r))
        cam, vao, _, svp = _structs(r, oracle)
        ref.append(dict(zip(("ao1", "stencil", "ray_min", "ray_max"),
                            oracle.svao_pass1(cam, vao, svp, depth, normals, r.sd_w, r.sd_h))))
        _assert_pass1(first[-1], ref[-1], ("first run", p))
    assert not np.array_equal(first[0]["ao"], first[-1]["ao"])
    for i in (0, len(points) - 2, 2):
        set_svao_point(r.vao, points[i])
        again = _pass1_snapshot(r)
        _assert_pass1(again, first[i], ("repeated run vs its first run", points[i]))
        _assert_pass1(again, ref[i], ("repeated run vs the oracle", points[i]))
    r.close()


def test_constant_cache_eviction_directions_and_kernels(oracle):
    """One VAOData, the cache's other key fields alternating: 8 / 16 directions x VAO / HBAO and 32 directions,
    five keys taken in turn twice, so that every call of the second round refills an evicted entry."""
    point = SVAO_SWEEP[1]
    keys = [(8, "vao"), (16, "vao"), (8, "hbao"), (16, "hbao"), (32, "vao")]
    rs, scene = [], None
    for nd, kernel in keys:
        r, scene = _renderer(point, num_directions=nd, ao_kernel=kernel, gpu_scene=rs[0].gscene if rs else None,
                             dev=rs[0].dev if rs else None)
        rs.append(r)
    rs[0].gbuffer()
    for r in rs[1:]:
        r.depth.copy_(rs[0].depth)
        r.normals.copy_(rs[0].normals)
    depth, normals = rs[0].numpy()["depth"], rs[0].numpy()["normals"]
    first = []
    for r, key in zip(rs, keys):
        first.append(_pass1_snapshot(r))
        cam, vao, _, svp = _structs(r, oracle)
        ref = dict(zip(("ao1", "stencil", "ray_min", "ray_max"),
                       oracle.svao_pass1(cam, vao, svp, depth, normals, r.sd_w, r.sd_h)))
        _assert_pass1(first[-1], ref, ("first round", key))
    for r, key, f in zip(rs, keys, first):
        _assert_pass1(_pass1_snapshot(r), f, ("second round", key))
    for r in rs:
        r.close()


# ---- e. depths outside the fast-division window, exact numerics

@pytest.mark.parametrize("kernel", ["vao", "hbao"])
def test_exact_numerics_out_of_window_depths(oracle, kernel):
    """Patches of depth exactly farZ, 1e7 (above pzHi), 1e-7 (below pzLo), 0 and an ordinary depth with a
    1-pixel checkerboard of 1e7 (waves mixing in-window and out-of-window lanes), with ssMaxRadius = 24 so
    that some of them clamp: the exact kernels' div_unscaled_*_ok guards and __ballot fallbacks (svao_math.h
    sample_init, svao_kernels.h) give the oracle's bits -- stencil, intervals, pass-1 AO, SD map and frame AO.
    (The pixels at depth 0 have NaN sample positions: their SD texel is UVToSDPixel's int(NaN) = 0 plus the
    guard, D3D's conversion, which the device's v_cvt_i32_f32 shares.)  Finite, non-negative depths only (NaN, inf and
    negative depths: test_gpu_numerics.py's degenerate inputs, by tolerance)."""
    import torch
    point = SVAO_DEFAULT_POINT[:2] + (24.0,) + SVAO_DEFAULT_POINT[3:]
    r, scene = _renderer(point, ao_kernel=kernel)
    cfg = r.cfg
    r.gbuffer()
    g0 = cfg.guard_band
    d = r.depth
    patch = torch.zeros_like(d, dtype=torch.bool)
    for (y0, y1, x0, x1), z in [((4, 24, 4, 44), cfg.far), ((30, 42, 60, 90), 1e7), ((50, 62, 10, 40), 1e-7),
                                ((70, 82, 50, 80), 0.0)]:
        d[g0 + y0:g0 + y1, g0 + x0:g0 + x1] = z
        patch[g0 + y0:g0 + y1, g0 + x0:g0 + x1] = True
    # the checkerboard: every other pixel of a 40 x 20 patch of an ordinary depth (the frame's median)
    y0, y1, x0, x1 = g0 + 60, g0 + 80, g0 + 110, g0 + 150
    yy, xx = torch.meshgrid(torch.arange(y0, y1, device=d.device), torch.arange(x0, x1, device=d.device), indexing="ij")
    d[y0:y1, x0:x1] = torch.where((yy + xx) % 2 == 0, torch.full_like(d[y0:y1, x0:x1], 1e7),
                                  d[g0:cfg.fb_h - g0, g0:cfg.fb_w - g0].median().expand(y1 - y0, x1 - x0))
    patch[y0:y1, x0:x1] = True
    torch.cuda.synchronize()
    assert int(patch.sum()) >= 2000
    g1, g = _gpu_frame(r)
    assert np.isfinite(g1["depth"]).all() and (g1["depth"] >= 0.0).all()
    clamped = radius_in_pixels(r.cam, r.vao, g1["depth"]) > np.float32(24.0)
    assert clamped[patch.cpu().numpy()].any() and (~clamped[patch.cpu().numpy()]).any()
    o = _oracle_frame(oracle, r, scene, g1)
    _assert_exact(r, g1, g, o, ("out-of-window depths", kernel))
    r.close()
