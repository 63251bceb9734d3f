"""The raster StochasticDepthMap pass without a GPU: the brute-force checker of the GPU tests
(tests/native/sd_raster_ref.c) pinned to the oracle's G-buffers, the conditions its base case must meet, and
the host side of the feature (ABI, header, graph planning, README)."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import sd_raster_checker as SR
from conftest import PKG, ROOT

W, H = SR.W, SR.H
HEADER = ROOT / "include" / "rsd.h"
SCRIPT = ROOT / "tests" / "graphs" / "svao_raster_sd.py"


@pytest.fixture(scope="module")
def checker(oracle, tmp_path_factory):
    return SR.build(oracle, tmp_path_factory.mktemp("sd_raster_ref"))


@pytest.fixture(scope="module")
def cases(oracle):
    return {k: SR.Case(oracle, k) for k in SR.SCENES}


def full_mask(oracle, checker, case, cull, linearize):
    """N = 1, Alpha = 1 (every fragment covers the sample), a zero depth map, no interval, no stencil."""
    prm = SR.params(N=1, alpha=1.0, cull=cull, linearize=linearize, ray_interval=False)
    m, cnt = SR.raster(oracle, checker, case, prm, np.zeros((H, W), np.float32), W, H)
    assert cnt["r_zero"] == cnt["ray_min"] == cnt["ray_max"] == cnt["stencilled"] == 0
    return m[0, :, :, 0], cnt


@pytest.mark.parametrize("kind,cull", [("opaque", 0), ("opaque", 1), ("opaque", 2), ("alpha", 1)])
def test_nearest_fragment_is_the_raster_gbuffer(oracle, checker, cases, kind, cull):
    """raster_depth is monotone, so the minimum over the fragments is the depth of the nearest hit."""
    c = cases[kind]
    m, cnt = full_mask(oracle, checker, c, cull, False)
    d, _ = oracle.gbuffer_raster(c.osc, c.ocam, W, H, cull)
    np.testing.assert_array_equal(SR.bits(m), SR.bits(d))
    assert int((d < 1.0).sum()) >= 100 and cnt["fragments"] >= int((d < 1.0).sum())
    if kind == "alpha":
        assert cnt["alpha"] > 0


@pytest.mark.parametrize("kind,cull", [("opaque", 1), ("alpha", 0)])
def test_linearized_value(oracle, checker, cases, kind, cull):
    c = cases[kind]
    m, _ = full_mask(oracle, checker, c, cull, True)
    z, _ = oracle.gbuffer(c.osc, c.ocam, W, H, cull)
    near, far = np.float32(c.ocam.nearZ), np.float32(c.ocam.farZ)
    want = (z - near) / (far - near)  # the cleared farZ of the G-buffer gives the cleared 1.0
    assert want.dtype == np.float32
    np.testing.assert_array_equal(SR.bits(m), SR.bits(want))


@pytest.mark.parametrize("divisor", [1, 2, 3])
def test_values_lie_behind_the_first_layer(oracle, checker, cases, divisor):
    c = cases["alpha"]
    d, _ = oracle.gbuffer_raster(c.osc, c.ocam, W, H, 0)
    sw, sh = -(-W // divisor), -(-H // divisor)
    m, cnt = SR.raster(oracle, checker, c, SR.params(N=4, cull=0, linearize=False, ray_interval=False), d, sw, sh)
    assert cnt["first_layer"] >= sw * sh // 4
    below = m < 1.0
    assert below.sum() >= 100
    if divisor == 1:  # the texel's own first layer
        first = np.broadcast_to(d[None, :, :, None], m.shape)
        assert (m[below] > first[below]).all()
    assert (m[below] > d.min()).all()


def test_base_case_exercises_every_rule(oracle, checker, cases):
    """The conditions of tests/test_gpu_sd_raster.py's base case, met by the checker alone."""
    B = SR.BASE
    c = cases[B["kind"]]
    fr = SR.oracle_frame(oracle, c, B["divisor"], B["radius"], B["N"], B["cull"])
    prm = SR.params(N=B["N"], alpha=B["alpha"], cull=B["cull"], use_stencil=True)
    m, cnt = SR.raster(oracle, checker, c, prm, fr.depth, fr.sd_w, fr.sd_h, fr.rmin, fr.rmax)
    for k in SR.COUNTERS[1:]:
        assert cnt[k] >= SR.BASE_MINIMUM, (k, cnt)
    assert cnt["stencilled"] == int((fr.rmax == 0).sum())
    assert (m[:, fr.rmax == 0] == 1.0).all()
    # an explicit mask takes precedence over rayMax
    mask = np.zeros((fr.sd_h, fr.sd_w), np.uint8)
    mask[:, : fr.sd_w // 2] = 1
    m2, cnt2 = SR.raster(oracle, checker, c, prm, fr.depth, fr.sd_w, fr.sd_h, fr.rmin, fr.rmax, stencil=mask)
    assert cnt2["stencilled"] == int((mask == 0).sum()) and (m2[:, mask == 0] == 1.0).all()
    # without the stencil format neither is read
    prm.use_stencil = 0
    _, cnt3 = SR.raster(oracle, checker, c, prm, fr.depth, fr.sd_w, fr.sd_h, fr.rmin, fr.rmax, stencil=mask)
    assert cnt3["stencilled"] == 0


# ---- the host side

def test_abi_exports_and_struct(tmp_path):
    from rsd import abi
    assert "rsd_sd_raster" in abi.EXPORTS
    assert abi.lib().rsd_abi_version() == 8
    text = HEADER.read_text()
    assert re.search(r"rsd_status\s+rsd_sd_raster\(", text) and "rsd_sd_raster_params" in text
    for field in ("sample_count", "alpha", "cull_mode", "linearize", "alpha_test", "implementation", "ray_interval",
                  "use_stencil"):
        assert field in [f[0] for f in abi.SDRasterParams._fields_]
    (tmp_path / "s.c").write_text('#include <stdio.h>\n#include "rsd.h"\nint main(void){'
                                  'printf("%zu\\n", sizeof(rsd_sd_raster_params));return 0;}\n')
    subprocess.run(["gcc", "-I", str(HEADER.parent), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    size = int(subprocess.run([str(tmp_path / "s")], capture_output=True, text=True).stdout)
    assert size == C.sizeof(abi.SDRasterParams) == C.sizeof(SR.Params)
    d = abi.SDRasterParams()  # StochasticDepthMap.h's defaults
    assert (d.sample_count, d.cull_mode, d.linearize, d.alpha_test, d.implementation, d.ray_interval,
            d.use_stencil) == (8, abi.CULL_BACK, 1, 1, abi.SD_DEFAULT, 1, 0)
    assert d.alpha == pytest.approx(0.2)
    out = subprocess.run(["nm", "-D", "--defined-only", str(PKG / "librsd.so")], capture_output=True, text=True).stdout
    assert re.search(r"\bT rsd_sd_raster\b", out)


def test_null_arguments_are_refused_without_a_gpu():
    from rsd import abi
    prm = abi.SDRasterParams()
    st = abi.lib().rsd_sd_raster(None, None, C.byref(prm), None, 0, 0, None, None, None, None, 0, 0, None)
    assert st == abi.ERR_INVALID_ARG and "rsd_sd_raster" in abi.last_error()


def test_pass_is_registered_and_reflects():
    from rsd import abi, graph as rg
    assert "StochasticDepthMap" in rg.plugin_types()
    z = np.zeros((32, 64), np.float32)  # planned only: never read
    for N, fmt, layers in [(1, "R32Float", 1), (2, "RG32Float", 1), (4, "RGBA32Float", 1), (8, "RGBA32Float", 2),
                           (16, "RGBA32Float", 4)]:
        g = rg.RenderGraph("sd")
        g.create_pass("SD", "StochasticDepthMap", {"SampleCount": N, "depthFormat": "D32FloatS8X24"})
        g.mark_output("SD.stochasticDepth")
        g.set_input("SD.depthMap", z.ctypes.data, 64, 32, abi.FMT_R32F)
        g.plan(32, 16)
        assert g.resources()["SD.stochasticDepth"] == (32, 16, layers, fmt)
        g.close()
    g = rg.RenderGraph("sd")  # SampleCount defaults to 8 (StochasticDepthMap.h)
    g.create_pass("SD", "StochasticDepthMap", {})
    g.mark_output("SD.stochasticDepth")
    g.set_input("SD.depthMap", z.ctypes.data, 64, 32, abi.FMT_R32F)
    g.plan(64, 32)
    assert g.resources()["SD.stochasticDepth"] == (64, 32, 2, "RGBA32Float")
    g.close()


@pytest.mark.parametrize("props", [{"SampleCount": 3}, {"Implementation": "ReservoirSampling"},
                                   {"Implementation": "KBuffer"}, {"depthFormat": "D24UnormS8"}])
def test_pass_refusals(props):
    from rsd import abi, graph as rg
    g = rg.RenderGraph("sd")
    z = np.zeros((32, 64), np.float32)
    with pytest.raises(abi.RsdError) as e:
        g.create_pass("SD", "StochasticDepthMap", props)
        g.mark_output("SD.stochasticDepth")
        g.set_input("SD.depthMap", z.ctypes.data, 64, 32, abi.FMT_R32F)
        g.plan(64, 32)
    assert e.value.status == abi.ERR_UNSUPPORTED
    g.close()


def test_rt_pass_still_refuses_its_raster_switch():
    from rsd import abi, graph as rg
    g = rg.RenderGraph("sd")
    with pytest.raises(abi.RsdError, match="raster variant"):
        g.create_pass("SD", "StochasticDepthMapRT", {"useRayPipeline": False})
    g.close()


def test_svao_raster_mode_plans():
    """tests/graphs/svao_raster_sd.py: no SD guard band in raster mode (SVAO.cpp:721), the SD size is
    ceil(size / divisor); with the selector at Ray the guard band is back."""
    from rsd import abi, graph as rg
    text = SCRIPT.read_text()
    g = rg.load_script(SCRIPT)["SVAORasterSD"]
    g.plan(W, H)
    assert g.resources()["SVAO.internalRayMax"] == (W, H, 1, "R32Uint")
    g.close()
    g = rg.load_script(text.replace("'stochMapDivisor': 1", "'stochMapDivisor': 2"))["SVAORasterSD"]
    g.plan(W, H)
    assert g.resources()["SVAO.internalRayMin"] == ((W + 1) // 2, (H + 1) // 2, 1, "R32Uint")
    g.close()
    g = rg.load_script(text.replace("'stochImpl': 'Raster'", "'stochImpl': 'Ray'"))["SVAORasterSD"]
    g.plan(W, H)
    assert g.resources()["SVAO.internalRayMax"] == (W + 32, H + 32, 1, "R32Uint")
    g.close()
    # raster mode without the non-linear depth: refused when planned
    g = rg.load_script(text.replace("    g.add_edge('GBufferRaster.depth', 'SVAO.gbufferDepth')\n", ""))["SVAORasterSD"]
    with pytest.raises(abi.RsdError, match="gbufferDepth") as e:
        g.plan(W, H)
    assert e.value.status == abi.ERR_UNSUPPORTED
    g.close()
    # the Ray default does not need it
    g = rg.load_script(text.replace("    g.add_edge('GBufferRaster.depth', 'SVAO.gbufferDepth')\n", "")
                       .replace("'stochImpl': 'Raster'", "'stochImpl': 'Ray'"))["SVAORasterSD"]
    g.plan(W, H)
    g.close()


def test_renderer_refuses_guard_band_jitter_and_16bit():
    """Renderer.sd_raster's argument checks come before any device work; a stand-in object carries the fields
    they read."""
    import types
    from rsd.frame import Renderer
    cfg = SR.frame_config()
    vao = types.SimpleNamespace(sdGuard=0)
    ok = types.SimpleNamespace(cfg=cfg, vao=vao, torch=None)
    for bad in (dict(jitter=True), dict(use_16bit=True)):
        import dataclasses
        r = types.SimpleNamespace(cfg=dataclasses.replace(cfg, **bad), vao=vao, torch=None)
        with pytest.raises(ValueError, match="sd_raster"):
            Renderer.sd_raster(r)
    with pytest.raises(ValueError, match="guard band"):
        Renderer.sd_raster(types.SimpleNamespace(cfg=cfg, vao=types.SimpleNamespace(sdGuard=4), torch=None))
    with pytest.raises(ValueError, match="sample_count"):
        Renderer.sd_raster(ok, sample_count=8)


def test_docs_mention_the_pass():
    readme = (ROOT / "README.md").read_text()
    assert "StochasticDepthMap" in readme and "rsd_sd_raster" in readme and "sd_raster" in readme
    design = (ROOT / "DESIGN.md").read_text()
    assert "rsd_sd_raster" in design and "stochImpl" in design
    assert "rsd_sd_raster" in (ROOT / "INTEGRATION.md").read_text()
