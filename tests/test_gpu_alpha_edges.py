"""GPU: the alpha test on the device at its texture, LOD and contract edges (csrc/alpha_test.h, csrc/tex_sample.h).

Every statement is bitwise against the oracle's frame (or the checkers built on the oracle's triangle and alpha test)
of the same inputs; tests/test_alpha_edges.py pins the oracle to tests/alpha_checker.py on the hits of these very
frames and proves that they reach every edge.  Output buffers lie between canaries.  The GPU's own output is never
the reference.
  * LOD 0: rsd_gbuffer (cull none / back), rsd_gbuffer_world, rsd_gbuffer_motion, rsd_depth_peel, rsd_sd_raster,
    rsd_rtao at 1 sample and pass 2 Raytraced on `shapes`, `uv_domain` and `thresholds`;
  * ray cone: rsd_sd_trace on `lod_ladder` and `uv_domain` under the quad, fused row, split and raster walks (the walk
    taken is asserted), the traversal and the wavefront order, implementations Default, CoverageMask and KBuffer,
    N = 4, and alpha_test = 0 as the control (the only trace the plan gives the hybrid walk);
  * the identities of `thresholds` on the device;
  * the dynamic path: refit, rebuild_bvh() and refit of the rebuilt tree of `uv_domain` and `shapes`, the motion
    G-buffer after it, and the records' flags words after the rebuild;
  * the texcoord contract's refusals (include/rsd.h rsd_alpha_desc.texcoords)."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest

import alpha_edge_scenes as E
import depth_peel_checker as DP
import mvec_checker as MV
import rtao_checker as RT
import sd_raster_checker as SR
from helpers import assert_canaries_intact, canary, to_oracle

pytestmark = pytest.mark.gpu
F = np.float32
bits = DP.bits


@pytest.fixture(scope="module")
def gpu(oracle):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rsd import abi
    from rsd.frame import Device, GpuScene
    dev = Device(0)
    g = types.SimpleNamespace(torch=torch, abi=abi, L=abi.lib(), dev=dev, scenes={}, GpuScene=GpuScene)
    for name in E.NAMES:
        g.scenes[name] = GpuScene(dev, E.build(name)[0])
    yield g
    torch.cuda.synchronize()
    for s in g.scenes.values():
        s.release()
    dev.close()


@pytest.fixture(scope="module")
def dp(oracle, tmp_path_factory):
    return DP.build(oracle, tmp_path_factory.mktemp("alpha_edges_peel"))


@pytest.fixture(scope="module")
def rt(oracle, tmp_path_factory):
    return RT.build(oracle, tmp_path_factory.mktemp("alpha_edges_rtao"))


@pytest.fixture(scope="module")
def sr(oracle, tmp_path_factory):
    return SR.build(oracle, tmp_path_factory.mktemp("alpha_edges_sd_raster"))


@pytest.fixture(scope="module")
def mv(oracle, tmp_path_factory):
    return MV.build(oracle, tmp_path_factory.mktemp("alpha_edges_gpu_mvec"))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _eq(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint8).reshape(got.shape + (-1,)) != want.view(np.uint8).reshape(want.shape + (-1,)))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())


def _case(oracle, scene, cfg):
    """What the checkers call a case: the scene, its oracle twin and the cameras of a frame of cfg."""
    cam, ocam = E.camera(oracle, cfg)
    return types.SimpleNamespace(scene=scene, cfg=cfg, cam=cam, ocam=ocam, osc=E.oscene(oracle, scene),
                                 has_alpha=scene.alpha is not None, size=(cfg.fb_w, cfg.fb_h))


def _gbuffer(gpu, gs, cam, cfg, cull, what):
    t = gpu.torch
    out = {"depth": canary(t, (cfg.fb_h, cfg.fb_w), t.float32), "normals": canary(t, (cfg.fb_h, cfg.fb_w), t.int16)}
    gpu.abi.check(gpu.L.rsd_gbuffer(gs.h, C.byref(cam), cfg.fb_w, cfg.fb_h, cull, _p(out["depth"].view),
                                    _p(out["normals"].view), None), "rsd_gbuffer")
    assert_canaries_intact(t, out, what)
    return out["depth"].numpy(), out["normals"].numpy().view(np.uint16)


def _sd_renderer(gpu, scene, gs, impl, hit_order=0, alpha_test=True):
    """A renderer whose SD trace runs from the camera: depth input 0, no intervals, no guard bands, no jitter; its SD
    map lies between canaries."""
    from rsd.frame import Renderer
    cfg = E.frame_config(guard=0, implementation=impl, hit_order=hit_order, ray_interval=False, alpha_test=alpha_test)
    r = Renderer(scene, cfg, dev=gpu.dev, gpu_scene=gs)
    r.depth.zero_()
    r.sd_canary = canary(gpu.torch, tuple(r.sd.shape), gpu.torch.float32)
    r.sd = r.sd_canary.view
    return r


def _sd_trace(gpu, r, what):
    r.sd_canary.fill()
    r.sd_trace()
    assert_canaries_intact(gpu.torch, {"sd": r.sd_canary}, what)
    return r.sd_canary.numpy()


def _oracle_sd(oracle, scene, impl, alpha_test=1):
    W, H = E.VISIBLE
    _, ocam = E.camera(oracle, E.frame_config(guard=0))
    return oracle.sd_trace(E.oscene(oracle, scene), ocam, E.sd_params(oracle, impl=impl, alpha_test=alpha_test),
                           np.zeros((H, W), F), None, None, W, H)[0]


# ------------------------------------------------------------------------------------------------ LOD 0

@pytest.mark.parametrize("name", E.LOD0_SCENES)
def test_gbuffers(oracle, rt, gpu, name):
    """rsd_gbuffer at cull none and back: the oracle's depth and normals.  rsd_gbuffer_world: the oracle's raster
    depth and face normals and the RTAO checker's world positions."""
    scene, _ = E.build(name)
    cfg = E.frame_config()
    c = _case(oracle, scene, cfg)
    W, H, t = cfg.fb_w, cfg.fb_h, gpu.torch
    for cull in (0, 1):
        z, n = oracle.gbuffer(c.osc, c.ocam, W, H, cull)
        gz, gn = _gbuffer(gpu, gpu.scenes[name], c.cam, cfg, cull, f"rsd_gbuffer {name} cull {cull}")
        _eq(gz, z, (name, cull, "depth"))
        _eq(gn, n, (name, cull, "normals"))
        out = {"depth": canary(t, (H, W), t.float32), "normal": canary(t, (H, W, 4), t.float32),
               "posW": canary(t, (H, W, 4), t.float32)}
        gpu.abi.check(gpu.L.rsd_gbuffer_world(gpu.scenes[name].h, C.byref(c.cam), W, H, cull, _p(out["depth"].view),
                                              _p(out["normal"].view), _p(out["posW"].view), None), "rsd_gbuffer_world")
        assert_canaries_intact(t, out, f"rsd_gbuffer_world {name} cull {cull}")
        d, nw = oracle.gbuffer_raster(c.osc, c.ocam, W, H, cull)
        _eq(out["depth"].numpy(), d, (name, cull, "world depth"))
        _eq(out["normal"].numpy(), nw, (name, cull, "world normal"))
        _eq(out["posW"].numpy(), RT.posw(oracle, rt, c, cull, width=W, height=H), (name, cull, "posW"))


@pytest.mark.parametrize("name", E.LOD0_SCENES)
def test_depth_peel_and_rtao(oracle, dp, rt, gpu, name):
    """rsd_depth_peel behind a first layer of depth 0 (separation 0.5): the nearest surface past 0.5 is the card where
    its hit is kept and the backdrop where it is not, so the peel's own alpha test decides every pixel.  (Behind the
    scene's real first layer it decides none: a kept card is the layer itself and a discarded one lies in front of it
    -- a peel with bu and bv swapped passed that version of this test.)  And rsd_rtao at one sample per pixel from the
    oracle's G-buffer.  The checkers' bits."""
    scene, _ = E.build(name)
    cfg = E.frame_config()
    c = _case(oracle, scene, cfg)
    W, H, t = cfg.fb_w, cfg.fb_h, gpu.torch
    z = np.zeros((H, W), F)
    prev = t.from_numpy(z).cuda()
    out = {"depth2": canary(t, (H, W), t.float32)}
    gpu.abi.check(gpu.L.rsd_depth_peel(gpu.scenes[name].h, C.byref(c.cam), W, H, 0, _p(prev), 0.5, 1,
                                       _p(out["depth2"].view), None), "rsd_depth_peel")
    assert_canaries_intact(t, out, f"rsd_depth_peel {name}")
    want = DP.peel(oracle, dp, c, 0, z, 0.5, 1, width=W, height=H)
    solid = types.SimpleNamespace(**{**vars(c), "has_alpha": False})
    assert (bits(want) != bits(DP.peel(oracle, dp, solid, 0, z, 0.5, 1, width=W, height=H))).sum() >= 1000
    _eq(out["depth2"].numpy(), want, (name, "depth2"))
    # RTAO: rays from the backdrop towards the cards' backs and from the cards
    _, nw = oracle.gbuffer_raster(c.osc, c.ocam, W, H, 0)
    pw = RT.posw(oracle, rt, c, 0, width=W, height=H)
    prm = gpu.abi.RTAOParams(max_t_hit=8.0 * float(-scene.positions[4, 2]) / 6.0, apply_exponential_falloff=False)
    v = C.c_float()
    gpu.abi.check(gpu.L.rsd_rtao_ray_t_max(C.byref(prm), C.byref(v)), "rsd_rtao_ray_t_max")
    tmax = F(v.value)
    ins = [t.from_numpy(np.ascontiguousarray(a)).cuda() for a in (pw, nw)]
    out = {"ambient": canary(t, (H, W), t.float32), "ray distance": canary(t, (H, W), t.float32)}
    gpu.abi.check(gpu.L.rsd_rtao(gpu.scenes[name].h, C.byref(prm), W, H, _p(ins[0]), _p(ins[1]), 0,
                                 _p(out["ambient"].view), _p(out["ray distance"].view), None, None), "rsd_rtao")
    assert_canaries_intact(t, out, f"rsd_rtao {name}")
    orig, d = RT.origins(rt, pw, nw, prm.normal_scale), RT.dirs(rt, pw, nw, 0)
    tr = RT.trace(oracle, rt, c.osc, True, orig, d, tmax)
    solid = RT.trace(oracle, rt, c.osc, False, orig, d, tmax)
    assert (bits(tr) != bits(solid)).sum() >= 100, "the alpha test decides too few AO rays"
    _eq(out["ambient"].numpy(), RT.ambient_no_falloff(tr[..., 0], prm.minimum_ambient_illumination), (name, "ambient"))
    _eq(out["ray distance"].numpy(), RT.ray_distance(tr, tmax), (name, "ray distance"))


@pytest.mark.parametrize("name", E.LOD0_SCENES)
def test_pass2_raytraced(oracle, gpu, name):
    """rsd_svao_pass2_raytraced after its own G-buffer and pass 1, exact numerics: the oracle's AO."""
    from rsd.frame import Renderer
    scene, _ = E.build(name)
    cfg = E.frame_config(secondary=gpu.abi.DEPTH_RAYTRACED, radius=2.0 * float(-scene.positions[4, 2]) / 6.0)
    r = Renderer(scene, cfg, dev=gpu.dev, gpu_scene=gpu.scenes[name])
    ao = canary(gpu.torch, tuple(r.ao.shape), gpu.torch.uint8)
    ao.view.zero_()
    r.ao = ao.view
    r.gbuffer()
    r.frame()
    assert_canaries_intact(gpu.torch, {"ao": ao}, f"pass 2 Raytraced {name}")
    g = r.numpy()
    cam, vao, svp = (to_oracle(r.cam, oracle.Camera), to_oracle(r.vao, oracle.VAOData),
                     to_oracle(r.svp, oracle.SVAOParams))
    osc = E.oscene(oracle, scene)
    z, n = oracle.gbuffer(osc, cam, cfg.fb_w, cfg.fb_h, cfg.cull_mode)
    _eq(g["depth"], z, (name, "depth"))
    ao1, st, _, _ = oracle.svao_pass1(cam, vao, svp, z, n, r.sd_w, r.sd_h)
    _eq(g["stencil"], st, (name, "stencil"))
    assert (st != 0).sum() >= 500, "pass 1 asks for too few rays"
    want = oracle.svao_pass2_raytraced(osc, cam, vao, svp, z, n, st, ao1, cull=cfg.cull_mode,
                                       ray_pipeline=int(cfg.ray_pipeline), alpha_test=1)
    solid = oracle.svao_pass2_raytraced(osc, cam, vao, svp, z, n, st, ao1, cull=cfg.cull_mode,
                                        ray_pipeline=int(cfg.ray_pipeline), alpha_test=0)
    assert (want != solid).sum() >= 20, "the alpha test decides too few AO rays"
    _eq(g["ao"], want, (name, "ao"))


@pytest.mark.parametrize("name", E.LOD0_SCENES)
def test_sd_raster(oracle, sr, gpu, name):
    """rsd_sd_raster behind a first layer of depth 0, without intervals and stencil, N = 4, linearised and not: the
    raster SD checker's bits.  Every card and the backdrop are fragments behind that layer, so the pass's own alpha
    test decides the card's fragment of every pixel (behind the scene's real first layer it would decide none, as in
    the depth peel); the checker without alpha data gives another map."""
    scene, _ = E.build(name)
    cfg = E.frame_config()
    c = _case(oracle, scene, cfg)
    W, H, t = cfg.fb_w, cfg.fb_h, gpu.torch
    z = np.zeros((H, W), F)
    depth = t.from_numpy(z).cuda()
    solid = types.SimpleNamespace(**{**vars(c), "has_alpha": False})
    for linearize in (True, False):
        prm = SR.params(N=4, alpha=None, cull=0, linearize=linearize, ray_interval=False, use_stencil=False)
        want, cnt = SR.raster(oracle, sr, c, prm, z, W, H)
        assert cnt["alpha"] >= 5000 and (bits(want) != bits(SR.raster(oracle, sr, solid, prm, z, W, H)[0])).sum() >= 5000
        out = {"sd": canary(t, want.shape, t.float32)}
        gp = gpu.abi.SDRasterParams.from_buffer_copy(prm)
        gpu.abi.check(gpu.L.rsd_sd_raster(gpu.scenes[name].h, C.byref(c.cam), C.byref(gp), _p(depth), W, H, None, None,
                                          None, _p(out["sd"].view), W, H, None), "rsd_sd_raster")
        assert_canaries_intact(t, out, f"rsd_sd_raster {name}")
        _eq(out["sd"].numpy(), want, (name, "raster SD map", linearize))
    _eq(depth.cpu().numpy(), z, (name, "the input depth"))


def _gbuffer_motion(gpu, gs, cam, cfg, cull, what):
    t, (W, H) = gpu.torch, (cfg.fb_w, cfg.fb_h)
    out = {"depth": canary(t, (H, W), t.float32), "normal": canary(t, (H, W, 4), t.float32),
           "mvec": canary(t, (H, W, 2), t.float32), "mvecW": canary(t, (H, W, 4), t.float32)}
    gpu.abi.check(gpu.L.rsd_gbuffer_motion(gs.h, C.byref(cam), C.byref(cam), W, H, cull, _p(out["depth"].view),
                                           _p(out["normal"].view), None, _p(out["mvec"].view), _p(out["mvecW"].view),
                                           None), "rsd_gbuffer_motion")
    assert_canaries_intact(t, out, what)
    return {k: o.numpy() for k, o in out.items()}


@pytest.mark.parametrize("name", E.LOD0_SCENES)
def test_gbuffer_motion(oracle, mv, gpu, name):
    """rsd_gbuffer_motion of the scene at rest (previous positions = current ones), cull none and back: depth and
    normal are the oracle's raster G-buffer, the motion vectors the checker's."""
    scene, _ = E.build(name)
    cfg = E.frame_config()
    c = _case(oracle, scene, cfg)
    gs = gpu.GpuScene(gpu.dev, scene, dynamic=True, motion=True)
    try:
        for cull in (0, 1):
            got = _gbuffer_motion(gpu, gs, c.cam, cfg, cull, f"rsd_gbuffer_motion {name} cull {cull}")
            d, nw = oracle.gbuffer_raster(c.osc, c.ocam, cfg.fb_w, cfg.fb_h, cull)
            _eq(got["depth"], d, (name, cull, "motion depth"))
            _eq(got["normal"], nw, (name, cull, "motion normal"))
            want = MV.run(oracle, mv, scene, scene.positions, scene.positions, c.cam, c.cam, (cfg.fb_w, cfg.fb_h), cull)
            _eq(got["mvec"], want["mvec"], (name, cull, "mvec"))
            _eq(got["mvecW"], want["mvec_w"], (name, cull, "mvecW"))
            # the alpha test decides this frame: with opaque cards the oracle's depth is another
            opaque = oracle.gbuffer_raster(E.oscene(oracle, E.opaque_variant(scene)), c.ocam, cfg.fb_w, cfg.fb_h, cull)[0]
            assert (bits(d) != bits(opaque)).sum() >= 1000
    finally:
        gpu.torch.cuda.synchronize()
        gs.release()


# ------------------------------------------------------------------------------------------------ the ray cone

_oracle_maps = {}


@pytest.mark.parametrize("walk", ["quad", "fused", "split", "raster"])
@pytest.mark.parametrize("impl", [0, 1, 3], ids=["Default", "CoverageMask", "KBuffer"])
@pytest.mark.parametrize("name", E.CONE_SCENES)
def test_sd_trace_canonical(oracle, gpu, monkeypatch, name, impl, walk):
    """rsd_sd_trace at the ray-cone LOD under RSD_TRACE_WALK = quad, fused, split and raster: the oracle's map, and
    the walk the trace took is the one asked for (rsd_counters.walk).  Two rows fall back, by csrc/sd_plan.cpp: the
    split and the raster walk need one chunk of K keys to decide a texel, which CoverageMask does not give
    (pl.split), so under CoverageMask both run the fused row walk -- asserted as such.
    Once per (scene, implementation), with the default plan: the alpha test on takes the fused row walk, never the
    hybrid -- the hybrid runs the specialised walks, which sd_plan.cpp allows only without the alpha test (specOk) --
    and alpha_test = 0, the control that the cards then count as opaque, takes the hybrid under Default (the
    specialised walks are Default's) and the fused row walk otherwise."""
    A = gpu.abi
    scene, _ = E.build(name)
    if (name, impl) not in _oracle_maps:
        _oracle_maps[name, impl] = (_oracle_sd(oracle, scene, impl), _oracle_sd(oracle, scene, impl, alpha_test=0))
    want, opaque = _oracle_maps[name, impl]
    assert (bits(want) != bits(opaque)).sum() >= 1000
    expected = {"quad": A.WALK_QUAD, "fused": A.WALK_FUSED, "split": A.WALK_SPLIT, "raster": A.WALK_RASTER}[walk]
    if impl == A.SD_COVERAGE_MASK and walk in ("split", "raster"):
        expected = A.WALK_FUSED
    monkeypatch.setenv("RSD_TRACE_WALK", walk)
    r = _sd_renderer(gpu, scene, gpu.scenes[name], impl)
    assert int(r.sd_trace(counters=True).walk) == expected, (name, impl, walk)
    _eq(_sd_trace(gpu, r, f"rsd_sd_trace {name} {impl} {walk}"), want, (name, impl, walk))
    if walk == "quad":
        monkeypatch.delenv("RSD_TRACE_WALK")
        assert int(r.sd_trace(counters=True).walk) == A.WALK_FUSED, "the default plan with the alpha test on"
        _eq(_sd_trace(gpu, r, f"rsd_sd_trace {name} {impl} default plan"), want, (name, impl, "default plan"))
        r0 = _sd_renderer(gpu, scene, gpu.scenes[name], impl, alpha_test=False)
        assert int(r0.sd_trace(counters=True).walk) == (A.WALK_HYBRID if impl == A.SD_DEFAULT else A.WALK_FUSED)
        _eq(_sd_trace(gpu, r0, f"rsd_sd_trace {name} {impl} alpha_test 0"), opaque, (name, impl, "alpha_test 0"))


@pytest.mark.parametrize("impl", [0, 1, 3], ids=["Default", "CoverageMask", "KBuffer"])
@pytest.mark.parametrize("name", E.CONE_SCENES)
def test_sd_trace_traversal_order(oracle, gpu, name, impl):
    """Hit order traversal: the oracle's walk of the device's own tree."""
    scene, _ = E.build(name)
    gs = gpu.scenes[name]
    r = _sd_renderer(gpu, scene, gs, impl, hit_order=gpu.abi.HIT_ORDER_TRAVERSAL)
    assert int(r.sd_trace(counters=True).walk) == gpu.abi.WALK_ORDERED
    got = _sd_trace(gpu, r, f"rsd_sd_trace traversal {name} {impl}")
    bvh, off = gs.export_bvh()
    W, H = E.VISIBLE
    want, _ = oracle.sd_trace_ordered(E.oscene(oracle, scene), bvh, off, to_oracle(r.cam, oracle.Camera),
                                      E.sd_params(oracle, impl=impl, hit_order=1), np.zeros((H, W), F), None, None, W, H)
    _eq(got, want, (name, impl, "traversal"))


@pytest.mark.parametrize("impl", [0, 1, 3], ids=["Default", "CoverageMask", "KBuffer"])
@pytest.mark.parametrize("name", E.CONE_SCENES)
def test_sd_trace_wavefront_order(oracle, gpu, name, impl):
    """Hit order wavefront (csrc/sd_walk_wavefront.hip's own alpha call site): the oracle's wavefront walk of the
    device's own tree, with librsd's pool bound min(208 - 3 wide_depth, 160)."""
    scene, _ = E.build(name)
    gs = gpu.scenes[name]
    r = _sd_renderer(gpu, scene, gs, impl, hit_order=gpu.abi.HIT_ORDER_WAVEFRONT)
    assert int(r.sd_trace(counters=True).walk) == gpu.abi.WALK_WAVEFRONT
    got = _sd_trace(gpu, r, f"rsd_sd_trace wavefront {name} {impl}")
    bvh, off = gs.export_bvh()
    soft = min(208 - 3 * int(gs.info.wide_depth), 160)
    W, H = E.VISIBLE
    want, _ = oracle.sd_trace_wavefront(E.oscene(oracle, scene), bvh, off, soft, to_oracle(r.cam, oracle.Camera),
                                        E.sd_params(oracle, impl=impl, hit_order=2), np.zeros((H, W), F), None, None,
                                        W, H)
    _eq(got, want, (name, impl, "wavefront"))
    assert (bits(want) != bits(_oracle_sd(oracle, scene, impl, alpha_test=0))).sum() >= 1000


# ------------------------------------------------------------------------------------------------ identities

def test_threshold_identities_on_the_device(oracle, gpu):
    """`thresholds` on the device equals the ORACLE's frames of the scene rewritten by its identities (kept cards
    opaque, discarding cards removed; for the Default reservoir only the kept half, tests/test_alpha_edges.py)."""
    scene, cards = E.build("thresholds")
    variant = E.identity_variant(scene, cards)
    kept_only = E.identity_variant(scene, [c for c in cards if c.identity == "kept"])
    cfg = E.frame_config()
    c = _case(oracle, variant, cfg)
    for cull in (0, 1):
        z, n = oracle.gbuffer(c.osc, c.ocam, cfg.fb_w, cfg.fb_h, cull)
        gz, gn = _gbuffer(gpu, gpu.scenes["thresholds"], c.cam, cfg, cull, "rsd_gbuffer thresholds")
        _eq(gz, z, ("identity depth", cull))
        _eq(gn, n, ("identity normals", cull))
    for impl, v in ((0, kept_only), (1, variant), (3, variant)):
        r = _sd_renderer(gpu, scene, gpu.scenes["thresholds"], impl)
        _eq(_sd_trace(gpu, r, f"identity SD {impl}"), _oracle_sd(oracle, v, impl), ("identity SD", impl))


# ------------------------------------------------------------------------------------------------ the dynamic path

@pytest.mark.parametrize("name", ["uv_domain", "shapes"])
def test_dynamic_scene_keeps_its_alpha_data(oracle, mv, gpu, name):
    """Upload as a dynamic scene; render after the upload, after update_positions (the cards move), after
    rebuild_bvh() and after a second update_positions on the rebuilt tree: G-buffer and KBuffer SD map are the
    oracle's of the moved scene and a fresh static upload's.  After the rebuild every record carries its primitive's
    flags word (the alpha bit included) and the bytes are host_bvh_lbvh's.  Last, the motion G-buffer between the two
    moved poses: the checker's motion vectors."""
    from rsd.frame import host_bvh_lbvh
    scene, _ = E.build(name)
    p1, p2 = E.moved(scene, 1), E.moved(scene, 2)
    cfg = E.frame_config()
    cam, ocam = E.camera(oracle, cfg)
    gs = gpu.GpuScene(gpu.dev, scene, dynamic=True, motion=True)
    fresh = None
    try:
        for step, pos in (("upload", scene.positions), ("moved", p1), ("rebuilt", p1), ("moved again", p2)):
            if step.startswith("moved"):
                gs.begin_frame()
                gs.update_positions(pos)
            elif step == "rebuilt":
                gs.rebuild_bvh()
                at = dataclasses.replace(scene, positions=pos)
                want, woff = host_bvh_lbvh(at)
                have, off = gs.export_bvh()
                assert off == woff
                _eq(have, want, (name, "rebuild"))
                recs = np.ascontiguousarray(have).view(np.uint32)[4 * off:][:12 * scene.indices.shape[0]].reshape(-1, 12)
                assert sorted(recs[:, 3].tolist()) == list(range(scene.indices.shape[0]))
                assert np.array_equal(recs[:, 7], scene.flags[recs[:, 3]]), "a record lost its primitive's flags"
                assert (recs[:, 7][recs[:, 3] >= 2] & E.FLAG_ALPHA_MASK).all()
            at = dataclasses.replace(scene, positions=np.ascontiguousarray(pos))
            osc = E.oscene(oracle, at)
            z, n = oracle.gbuffer(osc, ocam, cfg.fb_w, cfg.fb_h, 0)
            gz, gn = _gbuffer(gpu, gs, cam, cfg, 0, f"{name} {step}")
            _eq(gz, z, (name, step, "depth"))
            _eq(gn, n, (name, step, "normals"))
            sd = _oracle_sd(oracle, at, 3)
            r = _sd_renderer(gpu, at, gs, 3)
            _eq(_sd_trace(gpu, r, f"{name} {step} SD"), sd, (name, step, "SD"))
            if step != "upload":
                fresh = gpu.GpuScene(gpu.dev, at)
                fz, fn = _gbuffer(gpu, fresh, cam, cfg, 0, f"{name} {step} fresh")
                _eq(gz, fz, (name, step, "depth of a fresh upload"))
                _eq(gn, fn, (name, step, "normals of a fresh upload"))
                _eq(_sd_trace(gpu, _sd_renderer(gpu, at, fresh, 3), "fresh SD"), sd, (name, step, "fresh SD"))
                gpu.torch.cuda.synchronize()
                fresh.release()
                fresh = None
        # motion: previous positions p1 (the snapshot of the last begin_frame), current p2
        got = _gbuffer_motion(gpu, gs, cam, cfg, 0, f"rsd_gbuffer_motion {name}")
        W, H = cfg.fb_w, cfg.fb_h
        want = MV.run(oracle, mv, scene, p2, p1, cam, cam, (W, H), 0)
        _eq(got["mvec"], want["mvec"], (name, "mvec"))
        _eq(got["mvecW"], want["mvec_w"], (name, "mvecW"))
        d, nw = oracle.gbuffer_raster(E.oscene(oracle, dataclasses.replace(scene, positions=p2)), ocam, W, H, 0)
        _eq(got["depth"], d, (name, "motion depth"))
        _eq(got["normal"], nw, (name, "motion normal"))
        through = want["prim"] < 2
        assert through.sum() >= 500 and (~through).sum() >= 500 and bits(want["mvec"])[~through].any()
    finally:
        gpu.torch.cuda.synchronize()
        gs.release()
        if fresh is not None:
            fresh.release()


# ------------------------------------------------------------------------------------------------ refusals

BAD = [float("nan"), float("inf"), float("-inf"), 32769.0, -1e30]


def test_texcoord_contract(oracle, gpu):
    """NaN, +inf, -inf, 32769 and -1e30 in either texcoord component of a vertex of a textured alpha triangle: the
    static and the dynamic upload refuse, naming the vertex, and the device then uploads and renders a valid scene.
    The same values on a vertex that only the opaque backdrop names, and 32768 exactly on a textured alpha vertex,
    are accepted."""
    scene, _ = E.build("uv_domain")
    cfg = E.frame_config()
    c = _case(oracle, scene, cfg)
    z, n = oracle.gbuffer(c.osc, c.ocam, cfg.fb_w, cfg.fb_h, 0)
    vertex = int(scene.indices[5, 1])  # a card's vertex
    assert scene.flags[5] & E.FLAG_ALPHA_MASK
    for k, bad in enumerate(BAD):
        uv = scene.alpha.texcoords.copy()
        uv[vertex, k % 2] = bad
        broken = dataclasses.replace(scene, alpha=dataclasses.replace(scene.alpha, texcoords=uv))
        for dynamic in (False, True):
            with pytest.raises(RuntimeError, match=rf"vertex {vertex} \(triangle \d+\) has a texcoord"):
                gpu.GpuScene(gpu.dev, broken, dynamic=dynamic)
        ok = gpu.GpuScene(gpu.dev, scene)
        try:
            gz, gn = _gbuffer(gpu, ok, c.cam, cfg, 0, f"after the refusal of {bad}")
            _eq(gz, z, ("after a refusal", bad))
            _eq(gn, n, ("normals after a refusal", bad))
        finally:
            gpu.torch.cuda.synchronize()
            ok.release()
    # accepted: the backdrop's vertices (opaque triangles only) ...
    uv = scene.alpha.texcoords.copy()
    uv[:4, 0], uv[:4, 1] = BAD[:4], BAD[1:5]
    # ... and 32768 exactly on a card's vertex (the card's pixels then sample far away: the oracle's frame decides)
    uv[vertex] = [32768.0, -32768.0]
    edge = dataclasses.replace(scene, alpha=dataclasses.replace(scene.alpha, texcoords=uv))
    for dynamic in (False, True):
        gs = gpu.GpuScene(gpu.dev, edge, dynamic=dynamic)
        try:
            gz, gn = _gbuffer(gpu, gs, c.cam, cfg, 0, "the contract's edge")
            ez, en = oracle.gbuffer(E.oscene(oracle, edge), c.ocam, cfg.fb_w, cfg.fb_h, 0)
            _eq(gz, ez, ("32768", dynamic))
            _eq(gn, en, ("32768 normals", dynamic))
        finally:
            gpu.torch.cuda.synchronize()
            gs.release()
