"""CPU checks of the AO-resolve feature (rsd_ao_guided_blur, rsd_ao_variance_fix, the AOGuidedBlur and AOVarianceFix
graph passes): the passes are registered and reflect like the reference's, our graph script and the reference's
SVAO_depth.py and SAVO_record.py plan with them, the C entries refuse bad arguments without a GPU, the scalar
checker the GPU tests compare against (tests/native/ao_resolve_ref.c) gives the answers that can be known in
advance, and the inputs of the GPU tests reach every part of the shaders (asserted on the checker alone)."""
import ctypes as C
import shutil
from pathlib import Path

import numpy as np
import pytest

import ao_resolve_checker as AR
from conftest import ROOT

rsdgraph = pytest.importorskip("rsd.graph")
from rsd import abi  # noqa: E402

SCRIPT = ROOT / "tests" / "graphs" / "svao_dual_resolve.py"
REF_SCRIPTS = Path("/root/reference/scripts")
needs_gcc = pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
F = np.float32


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return AR.build(tmp_path_factory.mktemp("ao_resolve_ref"))


# ---------------------------------------------------------------------------------- passes, graphs, ABI

def test_passes_are_builtin():
    assert {"AOGuidedBlur", "AOVarianceFix"} <= set(rsdgraph.plugin_types())


def test_planning_a_dual_ao_resolve_chain():
    """SVAO (dualAO) -> DeinterleaveTexture -> AOGuidedBlur -> InterleaveTexture at 70 x 38: color is R8Unorm with the
    size and the layer count of ao2 (AOGuidedBlur.cpp:93-103); AOVarianceFix.color is shaped and formatted like its
    bright input (AOVarianceFix.cpp:83-93).  A stub declares neither."""
    g = rsdgraph.RenderGraph("resolve")
    g.create_pass("SVAO", "SVAO", {"dualAO": True, "secondaryDepthMode": "DualDepth"})
    for name in ("Z", "N", "B", "D"):
        g.create_pass(name, "Source", {})
    g.create_pass("DeinterleaveAO", "DeinterleaveTexture", {})
    g.create_pass("DeinterleaveZ", "DeinterleaveTexture", {})
    g.create_pass("AOGuidedBlur", "AOGuidedBlur", {"kernelRadius": 2, "clampResults": True, "enabled": True})
    g.create_pass("Interleave", "InterleaveTexture", {})
    g.create_pass("AOVarianceFix", "AOVarianceFix", {})
    g.add_edge("Z.z", "SVAO.depth")
    g.add_edge("N.n", "SVAO.normals")
    g.add_edge("SVAO.ao", "DeinterleaveAO.texIn")
    g.add_edge("Z.z", "DeinterleaveZ.texIn")
    g.add_edge("DeinterleaveAO.texOut", "AOGuidedBlur.ao2")
    g.add_edge("DeinterleaveZ.texOut", "AOGuidedBlur.lineardepth")
    g.add_edge("AOGuidedBlur.color", "Interleave.texIn")
    g.add_edge("B.b", "AOVarianceFix.bright")
    g.add_edge("D.d", "AOVarianceFix.dark")
    g.add_edge("DeinterleaveZ.texOut", "AOVarianceFix.lineardepth")
    g.mark_output("Interleave.texOut")
    g.mark_output("AOVarianceFix.color")
    g.plan(70, 38)
    res = g.resources()
    assert res["DeinterleaveAO.texOut"] == (18, 10, 16, "RG8Unorm")
    assert res["AOGuidedBlur.color"] == (18, 10, 16, "R8Unorm")
    assert res["Interleave.texOut"] == (70, 38, 1, "R8Unorm")
    assert res["B.b"] == (70, 38, 1, "R8Unorm") and res["D.d"][3] == "R8Unorm"  # stub producers: the declared formats
    assert res["AOVarianceFix.color"] == res["B.b"]
    order = g.execution_order()
    assert order.index("DeinterleaveAO") < order.index("AOGuidedBlur") < order.index("Interleave")
    # bright from a deinterleaved image: color follows it
    g.create_pass("DeinterleaveB", "DeinterleaveTexture", {})
    g.create_pass("Fix16", "AOVarianceFix", {})
    g.add_edge("B.b", "DeinterleaveB.texIn")
    g.add_edge("DeinterleaveB.texOut", "Fix16.bright")
    g.add_edge("DeinterleaveB.texOut", "Fix16.dark")
    g.add_edge("DeinterleaveZ.texOut", "Fix16.lineardepth")
    g.mark_output("Fix16.color")
    g.plan(70, 38)
    assert g.resources()["Fix16.color"] == (18, 10, 16, "R8Unorm")


def test_properties():
    g = rsdgraph.RenderGraph("props")
    g.create_pass("A", "AOGuidedBlur", {})  # AOGuidedBlur.h:87-90: enabled, radius 4, clampResults, local deviation
    g.create_pass("B", "AOGuidedBlur", {"kernelRadius": 20, "clampResults": False, "enabled": False, "localDeviation": False})
    for bad in (0, 21):
        with pytest.raises(abi.RsdError, match="kernelRadius"):
            g.create_pass(f"C{bad}", "AOGuidedBlur", {"kernelRadius": bad})
    g.create_pass("V", "AOVarianceFix", {})


def test_graph_script_plans():
    graphs = rsdgraph.load_script(SCRIPT)
    g = graphs["SVAODualResolve"]
    g.plan(70, 38)
    order = g.execution_order()
    for chain in (["GuardBand", "GBufferRaster", "LinearizeDepth", "SVAO", "DeinterleaveBrightDark", "AOGuidedBlur",
                   "InterleaveTexture0", "CrossBilateralBlurBL", "Ambient"],
                  ["LinearizeDepth", "DeinterleaveDepth", "AOGuidedBlur"]):
        assert [order.index(p) for p in chain] == sorted(order.index(p) for p in chain), order
    res = g.resources()
    assert res["SVAO.ao"] == (70, 38, 1, "RG8Unorm")
    assert res["DeinterleaveBrightDark.texOut"] == (18, 10, 16, "RG8Unorm")
    assert res["DeinterleaveDepth.texOut"] == (18, 10, 16, "R32Float")
    assert res["AOGuidedBlur.color"] == (18, 10, 16, "R8Unorm")
    assert res["InterleaveTexture0.texOut"] == (70, 38, 1, "R8Unorm")
    assert res["Ambient.out"] == (70, 38, 1, "RGBA32Float")
    assert "'enabled': True" in SCRIPT.read_text()  # what the GPU test replaces for the disabled case
    h = graphs["HBAOResolve"]
    h.plan(70, 38)
    res = h.resources()
    assert res["HBAO.ambientMap"] == (18, 10, 16, "RG8Unorm")
    assert res["AOGuidedBlur.color"] == (18, 10, 16, "R8Unorm")
    assert res["InterleaveAO.texOut"] == (70, 38, 1, "R8Unorm")


@pytest.mark.skipif(not REF_SCRIPTS.is_dir(), reason="reference scripts not present (GPU box)")
def test_reference_scripts_plan_with_the_real_passes():
    """scripts/SVAO_depth.py and scripts/SAVO_record.py at 2048 x 1208: the passes between DeinterleaveTexture and
    InterleaveTexture are the real ones; SAVO_record.py enables AOGuidedBlur on an R8Unorm map."""
    g = next(iter(rsdgraph.load_script(REF_SCRIPTS / "SVAO_depth.py").values()))
    g.plan(1920 + 128, 1080 + 128)
    order, res = g.execution_order(), g.resources()
    chain = ["SVAO", "DeinterleaveBrightDark", "AOGuidedBlur", "InterleaveTexture0", "CrossBilateralBlurBL"]
    assert [order.index(p) for p in chain] == sorted(order.index(p) for p in chain), order
    assert res["DeinterleaveBrightDark.texOut"][:3] == (512, 302, 16)
    assert res["AOGuidedBlur.color"] == (512, 302, 16, "R8Unorm")
    assert res["InterleaveTexture0.texOut"] == (2048, 1208, 1, "R8Unorm")
    g = next(iter(rsdgraph.load_script(REF_SCRIPTS / "SAVO_record.py").values()))
    g.plan(1920 + 128, 1080 + 128)
    order, res = g.execution_order(), g.resources()
    assert "AOGuidedBlur" in order and "AOVarianceFix" in order
    assert res["AOGuidedBlur.color"] == (512, 302, 16, "R8Unorm")
    assert res["AOVarianceFix.color"] == res["DeinterleaveBright.texOut"] == (512, 302, 16, "R8Unorm")
    assert res["InterleaveTexture1.texOut"] == (2048, 1208, 1, "R8Unorm")


@needs_gcc
def test_abi_mirror(tmp_path):
    """abi.AOGuidedBlurParams / AOVarianceFixParams have the layouts of the header's structs (sizes and offsets
    printed by a C program that includes it) and the pass's defaults; the new entries are exported."""
    import subprocess
    (tmp_path / "s.c").write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "rsd_graph.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", '
        "sizeof(rsd_ao_guided_blur_params), offsetof(rsd_ao_guided_blur_params, guard_band), "
        "offsetof(rsd_ao_guided_blur_params, layers), offsetof(rsd_ao_guided_blur_params, src_texel_bytes), "
        "sizeof(rsd_ao_variance_fix_params), offsetof(rsd_ao_variance_fix_params, layers));return 0;}\n")
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    sizes = [int(v) for v in subprocess.run([str(tmp_path / "s")], capture_output=True, text=True).stdout.split()]
    P, V = abi.AOGuidedBlurParams, abi.AOVarianceFixParams
    assert sizes == [C.sizeof(P), P.guard_band.offset, P.layers.offset, P.src_texel_bytes.offset, C.sizeof(V),
                     V.layers.offset] == [28, 8, 20, 24, 16, 12]
    p = P(70, 38)
    assert (p.kernel_radius, p.local_deviation, p.guard_band, p.width, p.height, p.layers, p.src_texel_bytes) == \
        (4, 1, 0, 70, 38, 16, 2)
    L = abi.lib()
    for name in ("rsd_ao_guided_blur", "rsd_ao_variance_fix", "rsd_ao_first_channel"):
        assert getattr(L, name) is not None and name in abi.GRAPH_EXPORTS
    assert L.rsd_abi_version() == 8


def test_arguments_are_checked():
    """Both entries refuse null pointers, an empty extent, a radius outside 1..20 and a texel size outside {1, 2}
    (status 1) and a layer count other than 1 or 16 (status 2), on the host, before any GPU work."""
    L = abi.lib()
    p = C.c_void_p(1 << 20)  # never dereferenced: the checks come first
    ok = dict(prm=abi.AOGuidedBlurParams(70, 38), src=p, z=p, ping=p, dst=p)

    def guided(**kw):
        a = {**ok, **kw}
        return L.rsd_ao_guided_blur(C.byref(a["prm"]) if a["prm"] is not None else None, a["src"], a["z"], a["ping"],
                                    a["dst"], None)

    P = abi.AOGuidedBlurParams
    bad = [dict(prm=None), dict(src=None), dict(z=None), dict(ping=None), dict(dst=None), dict(prm=P(0, 38)),
           dict(prm=P(70, 0)), dict(prm=P(70, 38, kernel_radius=0)), dict(prm=P(70, 38, kernel_radius=21)),
           dict(prm=P(70, 38, src_texel_bytes=0)), dict(prm=P(70, 38, src_texel_bytes=3)),
           dict(prm=P(70, 38, src_texel_bytes=4))]
    for b in bad:
        assert guided(**b) == abi.ERR_INVALID_ARG, b
        assert b"rsd_ao_guided_blur" in L.rsd_last_error(), b
    for layers in (0, 2, 4, 15, 17):
        assert guided(prm=P(70, 38, layers=layers)) == abi.ERR_UNSUPPORTED, layers
        assert b"layers" in L.rsd_last_error()
    # a guard band that leaves nothing inside the scissor draws nothing (and touches nothing)
    assert guided(prm=P(70, 38, guard_band=40)) == 0

    V = abi.AOVarianceFixParams
    okv = dict(prm=V(70, 38), b=p, d=p, z=p, dst=p)

    def variance(**kw):
        a = {**okv, **kw}
        return L.rsd_ao_variance_fix(C.byref(a["prm"]) if a["prm"] is not None else None, a["b"], a["d"], a["z"],
                                     a["dst"], None)

    for b in [dict(prm=None), dict(b=None), dict(d=None), dict(z=None), dict(dst=None), dict(prm=V(0, 38)),
              dict(prm=V(70, 0))]:
        assert variance(**b) == abi.ERR_INVALID_ARG, b
        assert b"rsd_ao_variance_fix" in L.rsd_last_error(), b
    for layers in (0, 2, 17):
        assert variance(prm=V(70, 38, layers=layers)) == abi.ERR_UNSUPPORTED, layers
    assert variance(prm=V(70, 38, guard_band=40)) == 0
    for args in [(None, 2, 10, p), (p, 2, 10, None), (p, 2, 0, p), (p, 0, 10, p), (p, 3, 10, p)]:
        assert L.rsd_ao_first_channel(*args, None) == abi.ERR_INVALID_ARG, args


# ---------------------------------------------------------------------------------- the checker, pinned

def _flat(shape, bright, dark, depth):
    return (np.full(shape + (2,), (bright, dark), np.uint8), np.full(shape, depth, F))


@needs_gcc
@pytest.mark.parametrize("local_deviation", [True, False])
@pytest.mark.parametrize("radius", AR.RADII)
def test_a_constant_image_comes_back_unchanged(checker, radius, local_deviation):
    """Constant (bright, dark) over a flat depth: every weighted mean is the constant to within an ulp, which the
    8-bit ping-pong image removes.  With the local deviation both deviations are far below DARK_EPSILON, so w = (1, 0)
    to within 1e-5 and the output is the bright byte.  Without it the 8-bit ping-pong image shows: its squares are the
    bytes 157 and 56, so sqrt|meansSq - means^2| is 0.023 and 0.043, not 0, and the output mixes bright and dark --
    the value worked out here in float32.  AOVarianceFix returns the bright byte."""
    src, z = _flat((1, 9, 9), 200, 120, 5.0)
    dst, ping, n = AR.guided_blur(checker, src, z, 9, 9, 0, radius, local_deviation)
    assert (ping[..., 0] == 200).all() and (ping[..., 1] == 120).all()
    sq = lambda c: int(np.floor(F(F(c / F(255)) * F(c / F(255))) * F(255) + F(0.5)))  # noqa: E731
    assert sq(F(200)) == 157 and sq(F(120)) == 56
    assert (ping[..., 2] == 157).all() and (ping[..., 3] == 56).all()
    if local_deviation:
        assert (dst == 200).all()
    else:
        b, d = F(200) / F(255), F(120) / F(255)
        ax, ay = np.sqrt(np.abs(F(157) / F(255) - b * b)), np.sqrt(np.abs(F(56) / F(255) - d * d))
        want = int(np.floor((b * (ay / (ax + ay)) + d * (ax / (ax + ay))) * F(255) + F(0.5)))
        assert 120 < want < 200 and (dst == want).all()
    assert n["written"] == 81 and n["tap_zero"] == 0 and n["fallback_x"] == 0 and n["fallback_y"] == 0
    assert n["tap_half"] == 2 * 81 * (2 * radius + 1)  # every tap of both passes has depth weight 1
    # the taps beyond the image are clamped (a tap on the outermost texel centre may count too: uv is accumulated)
    beyond = 2 * 9 * sum(max(0, radius - i) + max(0, radius - (8 - i)) for i in range(9))
    assert beyond <= n["tap_clamped"] <= beyond + 2 * 2 * 81
    assert n["ldev_raised"] == 81 and n["ldev_kept"] == 0
    out, nv = AR.variance_fix(checker, src[..., 0], src[..., 1], z, 9, 9, 0)
    assert (out == 200).all() and nv["adev_raised"] == 81 and nv["means_fallback"] == 0


@needs_gcc
def test_a_depth_step_leaves_the_two_sides_unmixed(checker):
    """Left half at depth 2 with (60, 30), right half at depth 4 with (240, 200): the relative depth across the step
    is 1 or 0.5, both weights exp(-500) and exp(-125) are 0 in float, so each side is a constant image of its own."""
    src, z = _flat((1, 8, 12), 60, 30, 2.0)
    src[:, :, 6:] = (240, 200)
    z[:, :, 6:] = 4.0
    for radius in (1, 4):
        dst, ping, n = AR.guided_blur(checker, src, z, 12, 8, 0, radius, True)
        assert (dst[:, :, :6] == 60).all() and (dst[:, :, 6:] == 240).all()
        assert (ping[:, :, :6, 1] == 30).all() and (ping[:, :, 6:, 1] == 200).all()
        assert n["tap_zero"] > 0 and n["fallback_x"] == 0
    out, nv = AR.variance_fix(checker, src[..., 0], src[..., 1], z, 12, 8, 0)
    assert (out[:, :, :6] == 60).all() and (out[:, :, 6:] == 240).all() and nv["tap_zero"] == 2 * 8


@needs_gcc
def test_a_centre_depth_of_zero_takes_the_fallback(checker):
    """max(0, 1.401298e-45) is the smallest denormal: a tap at depth 0 has 0 / denormal - 1 = -1 and any other tap
    inf - 1, so every weight is exp(-500) = 0 in float, weightSum < 1e-4 and the pixel keeps its own colour: the x
    pass writes (local, local^2), the y pass reads it back and its deviations are 0 -> the bright byte."""
    rng = np.random.default_rng(5)
    src = rng.integers(1, 256, (1, 6, 7, 2), dtype=np.uint8)
    z = np.full((1, 6, 7), 3.0, F)
    z[0, 2:4, 2:5] = 0.0
    dst, ping, n = AR.guided_blur(checker, src, z, 7, 6, 0, 2, True)
    assert n["fallback_x"] == 6 and n["fallback_y"] == 6
    assert np.array_equal(dst[0, 2:4, 2:5], src[0, 2:4, 2:5, 0])
    assert np.array_equal(ping[0, 2:4, 2:5, :2], src[0, 2:4, 2:5])
    # ... while a depth of the denormal itself is an ordinary depth: its own tap has weight 1
    z[0, 2:4, 2:5] = np.float32(1.401298e-45)
    assert z[0, 2, 2] > 0
    _, _, n = AR.guided_blur(checker, src, z, 7, 6, 0, 2, True)
    assert n["fallback_x"] == 0 and n["fallback_y"] == 0


@needs_gcc
def test_an_infinite_depth_meets_the_min(checker):
    """min(|z / z_0 - 1|, 1) decides only where the ratio is NaN: with a patch of depth +inf, inf / inf is NaN, HLSL's
    min returns the other operand, 1, the weight is 0 and the texels keep their own colour -- without the min the NaN
    would reach the output as 0.  A finite tap seen from an infinite centre has ratio 0: relative depth 1, weight 0.
    AOVarianceFix's saturate turns the same NaN into 0 and the weight into 1: the infinite texels average."""
    rng = np.random.default_rng(9)
    src = rng.integers(1, 256, (1, 6, 7, 2), dtype=np.uint8)
    z = np.full((1, 6, 7), 3.0, F)
    z[0, 2:4, 2:5] = np.inf
    dst, ping, n = AR.guided_blur(checker, src, z, 7, 6, 0, 2, True)
    assert n["fallback_x"] == 6 and n["fallback_y"] == 6
    assert np.array_equal(dst[0, 2:4, 2:5], src[0, 2:4, 2:5, 0]) and (dst[0, 2:4, 2:5] > 0).all()
    out, nv = AR.variance_fix(checker, src[..., 0], src[..., 1], z, 7, 6, 0)
    assert nv["tap_half"] >= 2 * 7  # the infinite neighbours of the infinite texels weigh 1


@needs_gcc
def test_on_an_r8_source_dark_is_zero(checker):
    """An R8Unorm source reads (bright, 0): the ping-pong image's second and fourth channels are 0, and the result
    equals that of the RG8Unorm source with a zero second channel -- not that of the bright channel duplicated."""
    s = AR.synthetic(70, 38, 16)
    dst1, ping1, n1 = AR.guided_blur(checker, s["bright"], s["depth"], 70, 38, 8, 2, True)
    zero = np.ascontiguousarray(np.stack([s["bright"], np.zeros_like(s["bright"])], -1))
    dst2, ping2, _ = AR.guided_blur(checker, zero, s["depth"], 70, 38, 8, 2, True)
    m = AR.inside(70, 38, 16, 8)
    assert np.array_equal(dst1, dst2) and np.array_equal(ping1, ping2)
    assert (ping1[m][:, 1] == 0).all() and (ping1[m][:, 3] == 0).all()
    twice = np.ascontiguousarray(np.stack([s["bright"], s["bright"]], -1))
    assert not np.array_equal(AR.guided_blur(checker, twice, s["depth"], 70, 38, 8, 2, True)[0], dst1)
    # with ldev.y = max(|0 - 0|, 0.01): c = bright * 0.01 / (ldev.x + 0.01), never above the bright byte
    assert (dst1[m] <= s["bright"][m]).all() and (dst1[m] < s["bright"][m]).any()
    assert n1["ldev_raised"] == n1["written"]


@needs_gcc
def test_the_scissor_and_the_uv_bounds(checker):
    """The scissor is guard_band / 4 on a 16-layer image and guard_band itself on a plain one; texels outside keep
    the fill in the output and in the ping-pong image; uvMin / uvMax come from the full-size frame."""
    for (W, H, L, g) in AR.CASES + [(70, 38, 1, 6)]:
        s = AR.synthetic(W, H, L)
        dst, ping, n = AR.guided_blur(checker, s["ao2"], s["depth"], W, H, g, 2, True)
        m = AR.inside(W, H, L, g)
        gl = g // 4 if L == 16 else g
        assert m.sum() == n["written"] == L * (m.shape[2] - 2 * gl) * (m.shape[1] - 2 * gl)
        assert (dst[~m] == AR.SENTINEL).all() and (ping[~m] == AR.SENTINEL).all()
        out, nv = AR.variance_fix(checker, s["bright"], s["dark"], s["depth"], W, H, g)
        assert (out[~m] == AR.SENTINEL).all() and nv["written"] == m.sum()
    # guard band 8 on 70 x 38: uvMin.x = 8.5 / 70 lies in layer texel 2 of 18 -- a tap left of it reads texel 2.  With
    # the bounds taken from the layer size (8.5 / 18) it would read texel 8.
    src, z = _flat((16, 10, 18), 100, 50, 5.0)
    src[:, :, 2] = (250, 50)
    dst, ping, _ = AR.guided_blur(checker, src, z, 70, 38, 8, 1, True)
    assert ping[0, 5, 3, 0] > 100 and ping[0, 5, 2, 0] > ping[0, 5, 3, 0]  # texel 2's own taps: 2 (clamped), 2, 3


# ---------------------------------------------------------------------------------- conditions on the inputs

@needs_gcc
@pytest.mark.parametrize("case", AR.CASES, ids=lambda c: "%dx%d_L%d_g%d" % c)
def test_the_base_inputs_populate_every_counter_class(checker, case):
    """A condition on the inputs of the GPU tests, asserted on the checker alone: with the RG8Unorm source, radius 2
    and the local deviation, every class the counters name occurs at least once in every case -- taps of depth weight
    exactly 0 and above 0.5, clamped taps, the weightSum fallback of both passes, ldev.y raised to DARK_EPSILON and
    not, an output exactly between two bytes; for AOVarianceFix also the means fallback."""
    W, H, L, g = case
    s = AR.synthetic(W, H, L)
    dst, ping, n = AR.guided_blur(checker, s["ao2"], s["depth"], W, H, g, 2, True)
    for k in AR.GUIDED_CLASSES:
        assert n[k] >= 1, (k, n)
    m = AR.inside(W, H, L, g)
    assert len(np.unique(dst[m])) > 30
    _, _, n0 = AR.guided_blur(checker, s["ao2"], s["depth"], W, H, g, 2, False)
    assert n0["adev_raised"] >= 1 and n0["adev_kept"] >= 1
    out, nv = AR.variance_fix(checker, s["bright"], s["dark"], s["depth"], W, H, g)
    for k in AR.VARIANCE_CLASSES:
        assert nv[k] >= 1, (k, nv)
    # the two settings, the two source formats and the radii give different images
    assert not np.array_equal(AR.guided_blur(checker, s["ao2"], s["depth"], W, H, g, 2, False)[0], dst)
    assert not np.array_equal(AR.guided_blur(checker, s["ao2"], s["depth"], W, H, g, 4, True)[0], dst)
    assert not np.array_equal(out, dst)


@needs_gcc
def test_radius_20_clamps_taps_of_every_pixel(checker):
    """Radius 20 exceeds every layer of the small cases: each pixel has clamped taps in both passes."""
    for (W, H, L, g) in AR.CASES[:1] + AR.CASES[2:]:
        s = AR.synthetic(W, H, L)
        _, _, n = AR.guided_blur(checker, s["ao2"], s["depth"], W, H, g, 20, True)
        assert n["tap_clamped"] >= 2 * n["written"]


@needs_gcc
def test_the_ping_pong_quantisation_is_visible(checker):
    """The y pass reads .zw of the 8-bit ping-pong image: recomputing the squares from its .xy (what a float
    ping-pong or a y pass that squares would amount to for these channels) changes outputs without the local
    deviation."""
    s = AR.synthetic(70, 38, 16)
    dst, ping, _ = AR.guided_blur(checker, s["ao2"], s["depth"], 70, 38, 8, 2, False)
    m = AR.inside(70, 38, 16, 8)
    v = ping[m].astype(F) / F(255)
    assert (np.abs(v[:, 2] - v[:, 0] * v[:, 0]) > 2.0 / 255).any()  # meansSq is not means^2: there is variance
