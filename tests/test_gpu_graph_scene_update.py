"""GPU: a render graph over a dynamic scene (rsd_graph_update_scene_positions).  tests/graphs/svao_hotpath.py is
executed, the scene's vertices are moved through the graph, and it is executed again: every output of the second
execute equals, bit for bit, a fresh graph over a fresh upload of the moved scene."""
import dataclasses

import numpy as np
import pytest

from conftest import ROOT
from helpers import small_frame_config

pytestmark = pytest.mark.gpu

SCRIPT = ROOT / "tests" / "graphs" / "svao_hotpath.py"
OUTPUTS = ["GBufferRaster.depth", "LinearizeDepth.linearDepth", "CompressNormals.normalOut", "SVAO.stencil",
           "SVAO.internalRayMin", "SVAO.internalRayMax", "SVAO.ao"]


def test_graph_renders_moved_geometry_on_its_next_execute():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rsd import abi, graph as rg
    from rsd.frame import Device, GpuScene, make_camera
    from rsd.scenes import make_scene
    cfg = small_frame_config()
    scene = make_scene("arcade_tiny", target_tris=3000)
    rng = np.random.default_rng(11)
    p1 = scene.positions + (0.02 * rng.standard_normal(scene.positions.shape)).astype(np.float32)
    p1[np.unique(scene.indices[-scene.indices.shape[0] // 8:])] += np.float32([0.4, 0.3, -0.5])
    moved = dataclasses.replace(scene, positions=np.ascontiguousarray(p1, np.float32))
    dev = Device(0)
    cam = make_camera(scene, cfg)
    scenes, graphs = [], []

    def run(gs, update=None):
        g = rg.load_script(SCRIPT)["SVAOHotPath"]
        graphs.append(g)
        g.set_scene(gs.h, cam)
        g.compile(cfg.fb_w, cfg.fb_h)
        g.execute()
        torch.cuda.synchronize()
        first = {n: g.output_tensor(n).cpu().numpy() for n in OUTPUTS}
        if update is not None:
            g.update_positions(update)
            g.execute()
            torch.cuda.synchronize()
        return first, {n: g.output_tensor(n).cpu().numpy() for n in OUTPUTS}

    try:
        scenes.append(GpuScene(dev, scene, dynamic=True))
        first, second = run(scenes[0], update=moved.positions)
        scenes.append(GpuScene(dev, moved))
        _, fresh = run(scenes[1])
        scenes.append(GpuScene(dev, scene))
        _, static = run(scenes[2])
        assert (fresh["SVAO.internalRayMax"].view(np.uint32) != 0).sum() > 0, "no SD rays: the frame is degenerate"
        for n in OUTPUTS:
            assert first[n].tobytes() == static[n].tobytes(), ("before the update: the static scene's frame", n)
            assert second[n].tobytes() == fresh[n].tobytes(), ("after the update: a fresh graph on the moved scene", n)
        assert second["SVAO.ao"].tobytes() != first["SVAO.ao"].tobytes(), "the motion does not show in the AO"
        g = graphs[2]
        with pytest.raises(abi.RsdError, match="not dynamic"):
            g.update_positions(moved.positions)
    finally:
        for g in graphs:
            g.close()
        for s in scenes:
            s.release()
        dev.close()
