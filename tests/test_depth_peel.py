"""CPU checks of the DepthPeeling feature (rsd_depth_peel, the DepthPeeling graph pass): the pass is
registered and reflects like the reference's, the C entry refuses bad arguments without a GPU, our
DualDepth graph script and the reference's SVAO scripts plan with it, and the brute-force checker the
GPU tests compare against (tests/native/depth_peel_ref.c) is pinned to the oracle's G-buffers."""
import ctypes as C
import shutil
from pathlib import Path

import numpy as np
import pytest

import depth_peel_checker as DP
from conftest import ROOT

rsdgraph = pytest.importorskip("rsd.graph")
from rsd import abi  # noqa: E402

SCRIPT = ROOT / "tests" / "graphs" / "svao_dual_peel.py"
REF_SCRIPTS = Path("/root/reference/scripts")
needs_gcc = pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")


@pytest.fixture(scope="session")
def checker(oracle, tmp_path_factory):
    return DP.build(oracle, tmp_path_factory.mktemp("depth_peel_ref"))


@pytest.fixture(scope="module")
def cases(oracle):
    return {k: DP.Case(oracle, k) for k in DP.SCENES}


def test_depth_peeling_is_a_builtin_pass():
    assert "DepthPeeling" in rsdgraph.plugin_types()


def test_depth_peel_arguments_are_checked():
    """rsd_depth_peel refuses null arguments, an empty extent, cull_mode 3 and linear_out 2 on the
    host (status 1 and a message naming the function), before any GPU work."""
    L = abi.lib()
    cam = abi.Camera()
    d = C.c_void_p(16)  # never dereferenced: the checks come first
    ok = dict(scene=d, cam=C.byref(cam), w=8, h=8, cull=1, prev=d, sep=0.5, lin=0, out=d)

    def call(**kw):
        a = {**ok, **kw}
        return L.rsd_depth_peel(a["scene"], a["cam"], a["w"], a["h"], a["cull"], a["prev"], a["sep"], a["lin"],
                                a["out"], None)

    for bad in (dict(scene=None), dict(cam=None), dict(prev=None), dict(out=None), dict(w=0), dict(h=0),
                dict(cull=3), dict(lin=2)):
        assert call(**bad) == abi.ERR_INVALID_ARG, bad
        assert b"rsd_depth_peel" in L.rsd_last_error(), bad


def test_dual_peel_script_plans():
    g = rsdgraph.load_script(SCRIPT)["SVAODualPeel"]
    g.plan(DP.W, DP.H)
    order = g.execution_order()
    assert order.index("LinearizeDepth") < order.index("DepthPeeling") < order.index("LinearizeDepth0") < \
        order.index("SVAO")
    assert "GuardBand" in order and "GBufferRaster" in order and "CompressNormals" in order
    assert g.resources()["DepthPeeling.depth2"] == (DP.W, DP.H, 1, "R32Float")
    assert g.resources()["LinearizeDepth0.linearDepth"] == (DP.W, DP.H, 1, "R32Float")


def test_depth_format_d16_is_refused():
    g = rsdgraph.RenderGraph("g")
    with pytest.raises(abi.RsdError, match="D32Float"):
        g.create_pass("P", "DepthPeeling", {"depthFormat": "D16Unorm"})
    with pytest.raises(abi.RsdError, match="unknown value 'Sideways'"):
        g.create_pass("Q", "DepthPeeling", {"cullMode": "Sideways"})
    g.create_pass("R", "DepthPeeling", {"cullMode": "None", "minSeparationDistance": 0.01, "someFutureKey": 1})


@pytest.mark.skipif(not REF_SCRIPTS.is_dir(), reason="reference scripts not present (GPU box)")
@pytest.mark.parametrize("name", ["SVAO.py", "SVAO_depth.py"])
def test_reference_scripts_plan_with_the_real_pass(name):
    g = next(iter(rsdgraph.load_script(REF_SCRIPTS / name).values()))
    g.plan(1920 + 128, 1080 + 128)
    assert "DepthPeeling" in g.execution_order()
    assert g.resources()["DepthPeeling.depth2"] == (2048, 1208, 1, "R32Float")


@needs_gcc
@pytest.mark.parametrize("kind,cull", [("opaque", 0), ("opaque", 1), ("opaque", 2), ("alpha", 1)])
def test_checker_is_pinned_to_the_oracle(oracle, checker, cases, kind, cull):
    """prev = 0, min_separation = 0 discards nothing (every hit has zlin >= nearZ > 0): the checker's
    first layer is the oracle's G-buffer bit for bit, in both output modes.  This ties the restated
    ray, culling, alpha test, (t, prim) tie-break and depth formula to the oracle."""
    c = cases[kind]
    zero = np.zeros((DP.H, DP.W), np.float32)
    raster = DP.peel(oracle, checker, c, cull, zero, 0.0, 0)
    linear = DP.peel(oracle, checker, c, cull, zero, 0.0, 1)
    want_r = oracle.gbuffer_raster(c.osc, c.ocam, DP.W, DP.H, cull)[0]
    want_l = oracle.gbuffer(c.osc, c.ocam, DP.W, DP.H, cull)[0]
    np.testing.assert_array_equal(DP.bits(raster), DP.bits(want_r))
    np.testing.assert_array_equal(DP.bits(linear), DP.bits(want_l))
    assert (want_r < 1.0).mean() >= 0.05  # the frame shows geometry
    if kind == "alpha":  # and alpha texels that fail: the masked scene differs from the opaque one
        from rsd.scenes import make_scene
        name, tris = DP.SCENES["alpha"]
        s = make_scene(name, target_tris=tris, alpha=False)
        solid = oracle.gbuffer(oracle.Scene(s.positions, s.indices, s.flags), c.ocam, DP.W, DP.H, cull)[0]
        assert (DP.bits(solid) != DP.bits(want_l)).sum() > 0


@needs_gcc
def test_checker_inputs_are_not_degenerate(oracle, checker, cases):
    """At min_separation 0.5, Back cull, prev = the oracle's G-buffer depth, the 75 x 45 frame of the
    reduced opaque scene holds both classes the GPU tests need, each on >= 5 % of the pixels
    (measured with the checker alone: 717 pixels with a second layer, 2658 cleared, of 3375)."""
    c = cases["opaque"]
    prev = oracle.gbuffer(c.osc, c.ocam, DP.W, DP.H, 1)[0]
    z2 = DP.peel(oracle, checker, c, 1, prev, 0.5, 1)
    far = np.float32(c.ocam.farZ)
    second, cleared = int((z2 < far).sum()), int((z2 == far).sum())
    print("second layer:", second, "cleared:", cleared, "of", z2.size)
    assert second + cleared == z2.size
    assert second >= 0.05 * z2.size and cleared >= 0.05 * z2.size
    assert (z2[z2 < far] > prev[z2 < far] + np.float32(0.5)).all()
