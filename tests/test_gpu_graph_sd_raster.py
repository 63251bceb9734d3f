"""GPU: the StochasticDepthMap graph pass, SVAO's raster SD mode (`stochImpl`) and Renderer.sd_raster against
the oracle's SVAO passes fed with the brute-force checker's map (tests/native/sd_raster_ref.c).  Exact
numerics, bitwise.  The frame is sd_raster_checker.BASE's: 75 x 45, the alpha scene, no culling, radius 6."""
import numpy as np
import pytest

import sd_raster_checker as SR
from conftest import ROOT

pytestmark = pytest.mark.gpu

W, H = SR.W, SR.H
B = SR.BASE
SCRIPT = ROOT / "tests" / "graphs" / "svao_raster_sd.py"


@pytest.fixture(scope="session")
def checker(oracle, tmp_path_factory):
    return SR.build(oracle, tmp_path_factory.mktemp("sd_raster_ref"))


@pytest.fixture(scope="module")
def gpu(oracle):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rsd.frame import Device, GpuScene

    class G:
        pass
    g = G()
    g.torch = torch
    g.dev = Device(0)
    g.case = SR.Case(oracle, B["kind"])
    g.scene = GpuScene(g.dev, g.case.scene)
    yield g
    g.scene.release()
    g.dev.close()


@pytest.fixture(scope="module")
def reference(oracle, checker, gpu):
    """Oracle pass 1 -> the checker's map (SVAO's raster properties, SVAO.cpp:158-176) -> oracle pass 2 with
    guard 0 and jitter off."""
    O, c = oracle, gpu.case
    fr = SR.oracle_frame(O, c, B["divisor"], B["radius"], B["N"], B["cull"])
    assert fr.svp.sd_jitter == 0 and fr.vao.sdGuard == 0
    prm = SR.params(N=B["N"], alpha=None, cull=B["cull"], linearize=True, use_stencil=True)
    sd, cnt = SR.raster(O, checker, c, prm, fr.depth, fr.sd_w, fr.sd_h, fr.rmin, fr.rmax)
    assert cnt["ray_max"] >= SR.BASE_MINIMUM and cnt["stencilled"] >= SR.BASE_MINIMUM
    ao = O.svao_pass2(c.ocam, fr.vao, fr.svp, fr.z, fr.normals, fr.stencil, sd, fr.ao1)
    assert (ao != fr.ao1).sum() >= 100, "pass 2 must refine this frame"
    return dict(frame=fr, sd=sd, ao=ao)


def run_graph(gpu, text, names):
    from rsd import graph as rg
    g = rg.load_script(text)["SVAORasterSD"]
    g.set_scene(gpu.scene.h, gpu.case.cam)
    g.compile(W, H)
    g.execute()
    g.execute()
    gpu.torch.cuda.synchronize()
    out = {n: g.output_tensor(n).cpu().numpy() for n in names}
    g.close()
    return out


def test_graph_svao_with_the_raster_producer(oracle, checker, gpu, reference):
    fr = reference["frame"]
    got = run_graph(gpu, SCRIPT.read_text(), ["SVAO.ao", "SVAO.stencil", "SVAO.internalRayMin", "SVAO.internalRayMax",
                                              "GBufferRaster.depth", "SDMap.stochasticDepth"])
    np.testing.assert_array_equal(SR.bits(got["GBufferRaster.depth"]).reshape(H, W), SR.bits(fr.depth))
    np.testing.assert_array_equal(got["SVAO.stencil"].reshape(H, W), fr.stencil)
    np.testing.assert_array_equal(got["SVAO.internalRayMin"].view(np.uint32).reshape(fr.sd_h, fr.sd_w), fr.rmin)
    np.testing.assert_array_equal(got["SVAO.internalRayMax"].view(np.uint32).reshape(fr.sd_h, fr.sd_w), fr.rmax)
    np.testing.assert_array_equal(got["SVAO.ao"].reshape(H, W), reference["ao"])
    # the standalone pass on the same depth: SampleCount 8, Alpha 0.2, D32Float (no stencil), no intervals
    prm = SR.params(N=8, alpha=0.2, cull=0, linearize=True, use_stencil=False)
    want, cnt = SR.raster(oracle, checker, gpu.case, prm, fr.depth, W, H)
    assert got["SDMap.stochasticDepth"].shape == want.shape == (2, H, W, 4)
    np.testing.assert_array_equal(SR.bits(got["SDMap.stochasticDepth"]), SR.bits(want))
    assert cnt["two_values"] >= SR.BASE_MINIMUM


def test_ray_selector_keeps_the_ray_traced_map(oracle, gpu, reference):
    """The same script with stochImpl 'Ray' and without the property: the RT producer's AO, as before."""
    from helpers import to_oracle
    from rsd.frame import make_vao, sd_params, svao_params
    O, c = oracle, gpu.case
    text = SCRIPT.read_text()
    ray = run_graph(gpu, text.replace("'stochImpl': 'Raster'", "'stochImpl': 'Ray'"), ["SVAO.ao"])["SVAO.ao"]
    default = run_graph(gpu, text.replace(", 'stochImpl': 'Raster'", ""), ["SVAO.ao"])["SVAO.ao"]
    np.testing.assert_array_equal(ray, default)
    # the RT frame of the oracle: SD guard band 16 px, jitter on (SVAO.h's defaults)
    cfg = SR.frame_config(B["divisor"], B["radius"], B["N"], B["cull"])
    cfg.sd_guard_px, cfg.jitter = 16, True
    vao, sd_w, sd_h = make_vao(cfg)
    ovao, svp = to_oracle(vao, O.VAOData), to_oracle(svao_params(cfg), O.SVAOParams)
    sdp = to_oracle(sd_params(cfg, vao.sdGuard), O.SDParams)
    fr = reference["frame"]
    ao1, st, rmin, rmax = O.svao_pass1(c.ocam, ovao, svp, fr.z, fr.normals, sd_w, sd_h)
    sd, _ = O.sd_trace(c.osc, c.ocam, sdp, fr.z, rmin, rmax, sd_w, sd_h)
    ao = O.svao_pass2(c.ocam, ovao, svp, fr.z, fr.normals, st, sd, ao1)
    np.testing.assert_array_equal(ray.reshape(H, W), ao)
    assert (ray.reshape(H, W) != reference["ao"]).any()


def test_raster_mode_needs_gbuffer_depth(gpu):
    from rsd import abi, graph as rg
    text = SCRIPT.read_text().replace("    g.add_edge('GBufferRaster.depth', 'SVAO.gbufferDepth')\n", "")
    g = rg.load_script(text)["SVAORasterSD"]
    g.set_scene(gpu.scene.h, gpu.case.cam)
    with pytest.raises(abi.RsdError, match="gbufferDepth") as e:
        g.compile(W, H)
    assert e.value.status == abi.ERR_UNSUPPORTED
    g.close()


def test_renderer_sd_raster(oracle, checker, gpu, reference):
    """clear_intervals(); pass1(); sd_raster(); pass2() on a renderer of the same frame."""
    from rsd.frame import Renderer
    O, c = oracle, gpu.case
    cfg = SR.frame_config(B["divisor"], B["radius"], B["N"], B["cull"])
    r = Renderer(c.scene, cfg, gpu_scene=gpu.scene, dev=gpu.dev)
    r.cam = c.cam
    r.gbuffer()
    r.clear_intervals()
    r.pass1()
    r.sd_raster()
    r.pass2()
    g = r.numpy()
    # the renderer's G-buffer is rsd_gbuffer's (the linear depth directly): the reference from its own bits
    z, n = O.gbuffer(c.osc, c.ocam, W, H, B["cull"])
    np.testing.assert_array_equal(SR.bits(g["depth"]), SR.bits(z))
    fr = reference["frame"]
    np.testing.assert_array_equal(SR.bits(r.raster_depth.cpu().numpy()), SR.bits(fr.depth))
    ao1, st, rmin, rmax = O.svao_pass1(c.ocam, fr.vao, fr.svp, z, n, r.sd_w, r.sd_h)
    prm = SR.params(N=B["N"], alpha=None, cull=B["cull"], linearize=True, use_stencil=True)
    sd, _ = SR.raster(O, checker, c, prm, fr.depth, r.sd_w, r.sd_h, rmin, rmax)
    np.testing.assert_array_equal(SR.bits(g["sd"]), SR.bits(sd))
    np.testing.assert_array_equal(g["ao"], O.svao_pass2(c.ocam, fr.vao, fr.svp, z, n, st, sd, ao1))
    # parameters override the config's: Alpha 0.2 gives BASE's map
    r.sd_raster(alpha=B["alpha"])
    prm = SR.params(N=B["N"], alpha=B["alpha"], cull=B["cull"], use_stencil=True)
    want, _ = SR.raster(O, checker, c, prm, fr.depth, r.sd_w, r.sd_h, rmin, rmax)
    np.testing.assert_array_equal(SR.bits(r.sd.cpu().numpy()), SR.bits(want))
