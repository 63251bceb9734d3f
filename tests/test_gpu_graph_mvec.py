"""GPU: GBufferRaster.mvec of a render graph over an animated scene that tracks its motion.  tests/graphs/svao_temporal.py
(SVAO -> blur -> TemporalAO -> TAA, both reading GBufferRaster.mvec) on tests/fixtures/turnstile.pyscene with a static
camera and three frames, the rig posed between them: the pass renders with rsd_gbuffer_motion and snapshots the
positions after it ran, so frame k's mvec is the checker's (tests/native/mvec_ref.c) for pose k-1 -> pose k.  The same
graph over the same scene without motion tracking writes what it wrote before: the camera-only vectors."""
import numpy as np
import pytest

import mvec_checker as MV
import skinning_checker
from conftest import ROOT
from helpers import small_frame_config, to_oracle

pytestmark = pytest.mark.gpu

SCRIPT = ROOT / "tests" / "graphs" / "svao_temporal.py"
TIMES = (0.25, 0.5, 0.9)


@pytest.fixture(scope="module")
def turnstile():
    from rsd.pyscene import load_pyscene
    scene = load_pyscene(ROOT / "tests" / "fixtures" / "turnstile.pyscene").build("turnstile")
    assert scene.rig is not None
    return scene, [skinning_checker.posed(scene.positions, scene.rig, scene.rig.matrices(t)) for t in TIMES]


def _same(got, want, what):
    bad = np.argwhere(MV.bits(got) != MV.bits(want))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def test_graph_mvec_follows_the_geometry(oracle, turnstile, tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rsd import abi, graph as rg
    from rsd.frame import Device, GpuScene, make_camera
    lib = MV.build(oracle, tmp_path_factory.mktemp("mvec_ref"))
    scene, poses = turnstile
    cfg = small_frame_config()
    size = (cfg.fb_w, cfg.fb_h)
    dev = Device(0)
    cam = make_camera(scene, cfg)
    scenes, graphs = [], []

    def graph(gs, extra=()):
        g = rg.load_script(SCRIPT)["SVAOTemporal"]
        graphs.append(g)
        for name in extra:
            g.mark_output(name)
        g.set_scene(gs.h, cam, rig=gs.rig)
        g.compile(*size)
        return g

    def frame(g, t, names):
        g.animate(t)
        g.execute()
        torch.cuda.synchronize()
        return {n: g.output_tensor(n).cpu().numpy() for n in names}

    try:
        # 1. the scene tracks its motion
        scenes.append(GpuScene(dev, scene, dynamic=True, motion=True))
        g = graph(scenes[0], extra=("GBufferRaster.mvecW",))
        names = ("GBufferRaster.mvec", "GBufferRaster.mvecW", "TemporalAO.aoOut", "AmbientTAA.colorOut")
        frames = [frame(g, t, names) for t in TIMES]
        assert scenes[0].motion_info().snapshots == 3, "one snapshot after each execute that followed an update"
        before = [scene.positions] + poses
        for k in range(3):  # frame 1 is measured against the positions at track_motion, the upload's
            want = MV.run(oracle, lib, scene, poses[k], before[k], cam, cam, size, abi.CULL_BACK)
            _same(frames[k]["GBufferRaster.mvec"], want["mvec"], f"frame {k + 1}: mvec")
            _same(frames[k]["GBufferRaster.mvecW"], want["mvec_w"], f"frame {k + 1}: mvecW")
            if k == 1:
                rotor = MV.bits(want["mvec_w"]).any(axis=-1)
                assert rotor.sum() > 50, "the rotor covers pixels of this frame"
                assert (np.abs(frames[k]["GBufferRaster.mvec"][rotor]).max(axis=-1) > 1e-4).mean() > 0.9, \
                    "the rotor's pixels carry its motion"
                assert np.abs(frames[k]["GBufferRaster.mvec"][~rotor]).max() < 1e-5, "static camera, static geometry"
        for f in frames:  # the chain runs through TemporalAO and TAA
            assert f["TemporalAO.aoOut"].any() and np.isfinite(f["AmbientTAA.colorOut"]).all()

        # 2. the same scene without motion tracking: today's bytes, the camera-only vectors of the posed scene
        scenes.append(GpuScene(dev, scene, dynamic=True))
        g2 = graph(scenes[1])
        oc = to_oracle(cam, oracle.Camera)
        for k, t in enumerate(TIMES[:2]):
            got = frame(g2, t, ("GBufferRaster.mvec",))["GBufferRaster.mvec"]
            osc = oracle.Scene(poses[k], scene.indices, scene.flags, scene.alpha)
            depth, _ = oracle.gbuffer_raster(osc, oc, size[0], size[1], abi.CULL_BACK)
            _same(got, oracle.motion_vectors_raster(oc, oc, depth), f"untracked frame {k + 1}")
            assert np.abs(got).max() < 1e-5, "camera-only: the rotor's motion does not show"
        assert scenes[1].motion_info().tracked == 0

        # 3. mvecW on a scene that does not track motion is Unsupported
        g3 = graph(scenes[1], extra=("GBufferRaster.mvecW",))
        with pytest.raises(abi.RsdError, match="tracks motion"):
            g3.execute()
    finally:
        torch.cuda.synchronize()
        for g in graphs:
            g.close()
        for s in scenes:
            s.release()
        dev.close()
