"""GPU: a glTF file end to end (rsd/gltf.py -> GpuScene.animate -> frames): the skinned, morphed cylinder of
tests/gltf_scenes.py at three times.  Positions bitwise against tests/morph_checker.py; the SVAO frame bitwise against a
fresh static upload of the checker's posed mesh (exact numerics, canonical hit order: the result does not depend on the
tree); motion vectors through rsd_gbuffer_motion, the call behind GBufferRaster.mvec."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import gltf_scenes
import morph_checker

pytestmark = pytest.mark.gpu

W, H = 75, 45


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rsd.frame import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cylinder(tmp_path_factory):
    from rsd.gltf import load_gltf
    w, info = gltf_scenes.cylinder()
    scene = load_gltf(w.save(tmp_path_factory.mktemp("gltf") / "cylinder.glb", "glb"))
    assert scene.rig.count == 16 and scene.rig.morph.entry_count == 15
    return scene, info


def _checker_positions(scene, t):
    rig, m = scene.rig, scene.rig.morph
    return morph_checker.posed(scene.positions, rig, rig.matrices(t), m.offsets, m.weight_ids, m.deltas,
                               rig.morph_weights(t))


def _cfg():
    from rsd.frame import FrameConfig
    cfg = FrameConfig(visible_w=W - 16, visible_h=H - 16, guard_band=8, divisor=1, sd_guard_px=16, radius=2.0,
                      numerics="exact", sd_samples=4)
    assert (cfg.fb_w, cfg.fb_h) == (W, H)
    return cfg


def test_animate_leaves_the_checkers_positions(gpu, cylinder):
    from rsd.frame import GpuScene
    scene, _ = cylinder
    gs = GpuScene(gpu, scene, dynamic=True)
    try:
        info = gs.morph_info()
        assert gs.rig is scene.rig and (info.attached, info.count, info.weight_count, info.entry_count) == (1, 16, 2, 15)
        for t in gltf_scenes.CYL_TIMES + (0.0,):
            gs.animate(t)
            have, want = morph_checker.export_positions(gs, scene.indices), _checker_positions(scene, t)
            assert _u32(have).tobytes() == _u32(want).tobytes(), t
        assert want.tobytes() == scene.positions.tobytes(), "the pose at the rest time is the soup"
    finally:
        gs.release()


@pytest.mark.parametrize("t", gltf_scenes.CYL_TIMES)
def test_animated_frame_equals_a_fresh_upload_of_the_checkers_mesh(gpu, cylinder, t, monkeypatch):
    from rsd.frame import GpuScene, Renderer
    monkeypatch.setenv("RSD_NUMERICS", "exact")
    scene, _ = cylinder
    moved = dataclasses.replace(scene, positions=_checker_positions(scene, t), rig=None)
    dyn, fresh = GpuScene(gpu, scene, dynamic=True), GpuScene(gpu, moved)
    try:
        out = []
        for sc, gs in ((scene, dyn), (moved, fresh)):
            r = Renderer(sc, _cfg(), dev=gpu, gpu_scene=gs)
            if gs is dyn:
                r.animate(t)
            r.gbuffer()
            r.frame()
            out.append(r.numpy())
        for key in ("depth", "normals", "ray_min", "ray_max", "sd", "ao"):
            assert out[0][key].shape == out[1][key].shape and out[0][key].tobytes() == out[1][key].tobytes(), (key, t)
        # depth is linear here: a miss holds the far plane (1000)
        assert (out[0]["depth"] < 100.0).sum() > 200 and (out[0]["sd"] != 0).any(), "the frame is degenerate"
    finally:
        dyn.release()
        fresh.release()


def test_motion_vectors_on_the_morphing_cap_and_the_static_floor(gpu, cylinder):
    import torch
    from rsd import abi
    from rsd.frame import GpuScene, look_at
    scene, _ = cylinder
    cam = look_at(scene.camera["pos"], scene.camera["target"], scene.camera["up"], _cfg())
    gs = GpuScene(gpu, scene, dynamic=True, motion=True)
    try:
        gs.animate(0.5)   # weights (0, 1)
        gs.begin_frame()
        gs.animate(1.0)   # weights (1, -0.5): target 0 lifts the cap
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")  # noqa: E731
        depth, normal, pos_w, mvec = z(H, W), z(H, W, 4), z(H, W, 4), z(H, W, 2)
        p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
        abi.check(abi.lib().rsd_gbuffer_motion(gs.h, C.byref(cam), C.byref(cam), W, H, 0, p(depth), p(normal), p(pos_w),
                                               p(mvec), None, None), "rsd_gbuffer_motion")
        torch.cuda.synchronize()
        d, y, mv = depth.cpu().numpy(), pos_w.cpu().numpy()[..., 1], np.abs(mvec.cpu().numpy()).max(axis=2)
        hit = d < 1.0
        floor, cap = hit & (np.abs(y + 0.5) < 1e-4), hit & (y > 1.0)
        assert floor.sum() > 100 and cap.sum() > 10, (floor.sum(), cap.sum())
        # mvec is the difference of two screen positions in [0, 1], each a handful of float32 operations rounded to at
        # most half an ulp of 1 (2^-24): still geometry with a still camera leaves that residue, not an exact 0.
        # 8 x 2^-24 bounds it; a moving surface is far above (a tenth of a pixel here is 1.3e-3)
        assert (mv[floor] <= 8 * 2.0**-24).all(), ("the static floor moves", mv[floor].max())
        assert (mv[cap] > 1e-3).all(), ("the morphing cap does not move", mv[cap].min())
    finally:
        gs.release()


def test_render_graph_animate_and_its_mvec(gpu, cylinder):
    """RenderGraph.set_scene(rig=...) / animate(t) / execute on the morphed rig: GBufferRaster.mvec of the second frame
    (0.5 -> 1.0) is non-zero on the morphing cap and, up to the residue explained above, zero on the static floor; the
    positions the graph's animate left are the checker's."""
    import torch
    from conftest import ROOT
    from helpers import small_frame_config
    from rsd import graph as rg
    from rsd.frame import GpuScene, make_camera
    scene, _ = cylinder
    cfg = small_frame_config()
    cam = make_camera(scene, cfg)
    gs = GpuScene(gpu, scene, dynamic=True, motion=True)
    g = rg.load_script(ROOT / "tests" / "graphs" / "svao_temporal.py")["SVAOTemporal"]
    try:
        g.mark_output("GBufferRaster.posW")
        g.set_scene(gs.h, cam, rig=gs.rig)
        g.compile(cfg.fb_w, cfg.fb_h)
        for t in (0.5, 1.0):
            g.animate(t)
            g.execute()
            torch.cuda.synchronize()
        have = morph_checker.export_positions(gs, scene.indices)
        assert _u32(have).tobytes() == _u32(_checker_positions(scene, 1.0)).tobytes()
        assert gs.dynamic_info().updates == 2 and gs.motion_info().snapshots == 2
        mv = np.abs(g.output_tensor("GBufferRaster.mvec").cpu().numpy()).max(axis=-1)
        pos = g.output_tensor("GBufferRaster.posW").cpu().numpy()
        y, hit = pos[..., 1], np.abs(pos[..., :3]).max(axis=-1) > 0
        floor, cap = hit & (np.abs(y + 0.5) < 1e-4), hit & (y > 1.0)
        assert floor.sum() > 100 and cap.sum() > 10, (floor.sum(), cap.sum())
        assert (mv[floor] <= 8 * 2.0**-24).all(), ("the static floor moves", mv[floor].max())
        assert (mv[cap] > 1e-3).all(), ("the morphing cap does not move", mv[cap].min())
    finally:
        torch.cuda.synchronize()
        g.close()
        gs.release()


def test_a_rig_whose_targets_are_all_zero_animates(gpu, tmp_path):
    """Its table has no entries, so none is attached, and animate poses it like a rig without a table."""
    import gltf_writer as G
    from rsd.frame import GpuScene
    from rsd.gltf import load_gltf
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    w = G.Writer()
    mesh = w.add("meshes", {"weights": [1.0], "primitives": [{"attributes": {"POSITION": w.accessor(pos)},
                                                              "targets": [{"POSITION": w.accessor(np.zeros((3, 3)))}]}]})
    w.add("nodes", G.trs_node([0, 0, 3], mesh=mesh))
    scene = load_gltf(w.save(tmp_path / "z.gltf"))
    gs = GpuScene(gpu, scene, dynamic=True)
    try:
        assert gs.rig_info().count == 3 and gs.morph_info().attached == 0
        gs.animate(0.3)
        have = morph_checker.export_positions(gs, scene.indices)
        assert _u32(have).tobytes() == _u32(scene.positions).tobytes()
    finally:
        gs.release()
