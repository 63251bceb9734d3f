"""GPU: a render graph and a Renderer over an animated scene.  tests/fixtures/turnstile.pyscene is built, uploaded as a
dynamic scene with its rig and animated to time t (RenderGraph.animate / Renderer.animate: keyframes and hierarchy on
the host, rsd_scene_update_pose on the device); the AO equals, bit for bit, the same graph (the same renderer) over a
static upload of the positions tests/skinning_checker.py computes for the controller's matrices at t."""
import dataclasses

import numpy as np
import pytest

import skinning_checker
from conftest import ROOT
from helpers import small_frame_config

pytestmark = pytest.mark.gpu

SCRIPT = ROOT / "tests" / "graphs" / "svao_hotpath.py"
TIMES = (0.37, 1.9)  # 1.9 is past the last keyframe (1.5): both animations cycle


@pytest.fixture(scope="module")
def turnstile():
    from rsd.pyscene import load_pyscene
    scene = load_pyscene(ROOT / "tests" / "fixtures" / "turnstile.pyscene").build("turnstile")
    assert scene.rig is not None
    at = {t: dataclasses.replace(scene, rig=None, positions=skinning_checker.posed(scene.positions, scene.rig,
                                                                                  scene.rig.matrices(t)))
          for t in TIMES}
    return scene, at


def test_graph_animate_renders_the_scene_at_that_time(turnstile):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rsd import graph as rg
    from rsd.frame import Device, GpuScene, make_camera
    scene, at = turnstile
    cfg = small_frame_config()
    dev = Device(0)
    cam = make_camera(scene, cfg)
    scenes, graphs = [], []

    def graph(gs):
        g = rg.load_script(SCRIPT)["SVAOHotPath"]
        graphs.append(g)
        g.set_scene(gs.h, cam, rig=gs.rig)
        g.compile(cfg.fb_w, cfg.fb_h)
        return g

    def ao(g):
        g.execute()
        torch.cuda.synchronize()
        return g.output_tensor("SVAO.ao").cpu().numpy(), g.output_tensor("SVAO.internalRayMax").cpu().numpy()

    try:
        scenes.append(GpuScene(dev, scene, dynamic=True))
        g = graph(scenes[0])
        rest, _ = ao(g)
        seen = [rest.tobytes()]
        for t in TIMES:
            g.animate(t)
            moving, _ = ao(g)
            scenes.append(GpuScene(dev, at[t]))
            still, rays = ao(graph(scenes[-1]))
            assert (rays.view(np.uint32) != 0).sum() > 0, "no SD rays: the frame is degenerate"
            assert moving.tobytes() == still.tobytes(), t
            assert moving.tobytes() not in seen, "the motion does not show in the AO"
            seen.append(moving.tobytes())
        with pytest.raises(ValueError, match="no rig"):
            graphs[-1].animate(0.5)
    finally:
        for g in graphs:
            g.close()
        for s in scenes:
            s.release()
        dev.close()


def test_renderer_animate_renders_the_scene_at_that_time(turnstile):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rsd.frame import Renderer
    scene, at = turnstile
    t = TIMES[0]
    cfg = dataclasses.replace(small_frame_config(), numerics="exact")
    r = Renderer(scene, cfg, dynamic=True)
    s = Renderer(at[t], cfg, dev=r.dev)
    try:
        r.gbuffer()
        r.frame()
        rest = r.numpy()["ao"].tobytes()
        r.animate(t)
        r.gbuffer()
        r.frame()
        s.gbuffer()
        s.frame()
        a, b = r.numpy(), s.numpy()
        for key in ("depth", "sd", "ao"):
            assert a[key].tobytes() == b[key].tobytes(), key
        assert a["ao"].tobytes() != rest, "the motion does not show in the AO"
    finally:
        s.close()
        r.close()
        r.dev.close()
