"""CPU checks of the HBAO feature (rsd_hbao, rsd_hbao_noise_table, rsd_cross_bilateral_blur_src, the HBAO graph
pass): the pass is registered and reflects like the reference's, our graph script and the reference's HBAO.py
plan with it, the C entries refuse bad arguments without a GPU, the noise table is MT19937(0)'s, the scalar
checker the GPU tests compare against (tests/native/hbao_ref.c) gives the answers that can be known in advance,
and the inputs of the GPU tests reach every part of the shader (asserted on the checker alone)."""
import ctypes as C
import shutil
from pathlib import Path

import numpy as np
import pytest

import hbao_checker as HB
from conftest import ROOT

rsdgraph = pytest.importorskip("rsd.graph")
from rsd import abi  # noqa: E402

SCRIPT = ROOT / "tests" / "graphs" / "hbao.py"
REF_SCRIPTS = Path("/root/reference/scripts")
needs_gcc = pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
F = np.float32


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return HB.build(tmp_path_factory.mktemp("hbao_ref"))


# ---------------------------------------------------------------------------------- pass, graphs, ABI

def test_hbao_is_a_builtin_pass():
    assert "HBAO" in rsdgraph.plugin_types()


def _hbao_graph(props, depth2=True):
    g = rsdgraph.RenderGraph("hbao")
    g.create_pass("H", "HBAO", props)
    for name in ("Z", "Z2", "N"):
        g.create_pass(name, "Source", {})
    g.add_edge("Z.z", "H.depth")
    if depth2:
        g.add_edge("Z2.z", "H.depth2")
    g.add_edge("N.n", "H.normals")
    g.mark_output("H.ambientMap")
    return g


def test_reflection():
    """HBAO::reflect (HBAO.cpp:104-125): 16 RG8Unorm layers of ceil(w/4) x ceil(h/4) out; depth, depth2 and normals
    in (stub producers take the declared formats).  depth2 may stay unconnected unless the mode is DualDepth; the
    StochasticDepth mode is refused when the graph is planned."""
    g = _hbao_graph({"radius": 1.0, "depthMode": "SingleDepth", "depthBias": 0.1, "exponent": 2.0})
    g.plan(150, 90)
    res = g.resources()
    assert res["H.ambientMap"] == (38, 23, 16, "RG8Unorm")
    assert res["Z.z"][3] == "R32Float" and res["Z2.z"][3] == "R32Float" and res["N.n"][3] == "RGBA32Float"
    g.plan(64, 48)
    assert g.resources()["H.ambientMap"] == (16, 12, 16, "RG8Unorm")
    _hbao_graph({"depthMode": "SingleDepth"}, depth2=False).plan(150, 90)
    _hbao_graph({}, depth2=False).plan(150, 90)  # the default mode is SingleDepth (HBAO.h:67)
    _hbao_graph({"depthMode": "DualDepth"}).plan(150, 90)
    with pytest.raises(abi.RsdError, match="H.depth2"):
        _hbao_graph({"depthMode": "DualDepth"}, depth2=False).plan(150, 90)
    with pytest.raises(abi.RsdError, match="SingleDepth or DualDepth") as e:
        _hbao_graph({"depthMode": "StochasticDepth"}).plan(150, 90)
    assert e.value.status == abi.ERR_UNSUPPORTED
    with pytest.raises(abi.RsdError, match="radius"):
        _hbao_graph({"radius": 0.0})
    _hbao_graph({"enabled": False}).plan(150, 90)  # librsd's optional property


def test_hbao_script_plans():
    g = rsdgraph.load_script(SCRIPT)["HBAOGraph"]
    g.plan(150, 90)
    order = g.execution_order()
    for chain in (["GuardBand", "GBufferRaster", "LinearizeDepth", "DeinterleaveDepth", "HBAO", "InterleaveAO", "BlurAO",
                   "Ambient"],
                  ["LinearizeDepth", "DepthPeeling", "LinearizeDepth2", "DeinterleaveDepth2", "HBAO"]):
        assert [order.index(p) for p in chain] == sorted(order.index(p) for p in chain), order
    res = g.resources()
    assert res["DeinterleaveDepth.texOut"] == (38, 23, 16, "R32Float")
    assert res["DeinterleaveDepth2.texOut"] == (38, 23, 16, "R32Float")
    assert res["HBAO.ambientMap"] == (38, 23, 16, "RG8Unorm")
    assert res["InterleaveAO.texOut"] == (150, 90, 1, "RG8Unorm")
    assert res["BlurAO.colorOut"] == (150, 90, 1, "R8Unorm")
    assert res["Ambient.out"] == (150, 90, 1, "RGBA32Float")
    assert "'depthMode': 'DualDepth'" in SCRIPT.read_text()  # what the GPU test replaces per mode


@pytest.mark.skipif(not REF_SCRIPTS.is_dir(), reason="reference scripts not present (GPU box)")
def test_reference_script_plans_with_the_real_pass():
    """scripts/HBAO.py: the pass in the middle is the real one (a stub has no reflection, so its output would be
    shaped by its consumer), and the blur's colour input is the interleaved RG8Unorm map."""
    g = next(iter(rsdgraph.load_script(REF_SCRIPTS / "HBAO.py").values()))
    g.plan(1920 + 128, 1080 + 128)
    order = g.execution_order()
    chain = ["LinearizeDepth", "DeinterleaveDepth", "HBAO", "InterleaveTexture0", "CrossBilateralBlurBL", "Ambient"]
    assert [order.index(p) for p in chain] == sorted(order.index(p) for p in chain), order
    res = g.resources()
    assert res["HBAO.ambientMap"] == (512, 302, 16, "RG8Unorm")
    assert res["InterleaveTexture0.texOut"] == (2048, 1208, 1, "RG8Unorm")
    assert res["CrossBilateralBlurBL.colorOut"] == (2048, 1208, 1, "R8Unorm")
    assert res["DeinterleaveTexture.texOut"] == (512, 302, 16, "R32Float")  # HBAO.depth2 (unused in SingleDepth)


@needs_gcc
def test_abi_mirror(tmp_path):
    """abi.HBAOParams has rsd_hbao_params' layout (sizes and offsets printed by a C program that includes the
    header) and defaults; the new entries are exported."""
    import subprocess
    (tmp_path / "s.c").write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "rsd_graph.h"\nint main(void){printf("%zu %zu %zu %zu\\n", '
        "sizeof(rsd_hbao_params), offsetof(rsd_hbao_params, depth_mode), offsetof(rsd_hbao_params, guard_band), "
        "offsetof(rsd_hbao_params, rand));return 0;}\n")
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    sizes = [int(v) for v in subprocess.run([str(tmp_path / "s")], capture_output=True, text=True).stdout.split()]
    P = abi.HBAOParams
    assert sizes == [C.sizeof(P), P.depth_mode.offset, P.guard_band.offset, P.rand.offset] == [276, 12, 16, 20]
    p = abi.HBAOParams()
    assert (p.radius, p.power_exponent, p.depth_mode, p.guard_band) == (1.0, 2.0, 0, 0)
    assert p.ndotv_bias == float(F(0.1))
    L = abi.lib()
    for name in ("rsd_hbao", "rsd_hbao_noise_table", "rsd_cross_bilateral_blur_src"):
        assert getattr(L, name) is not None
    assert {"rsd_hbao", "rsd_hbao_noise_table"} <= set(abi.EXPORTS)
    assert "rsd_cross_bilateral_blur_src" in abi.GRAPH_EXPORTS
    assert L.rsd_abi_version() == 8
    custom = abi.HBAOParams(rand=[[i, 1, 2, 3] for i in range(16)])
    assert custom.rand[5][0] == 5.0 and custom.rand[15][3] == 3.0


def test_arguments_are_checked():
    """rsd_hbao refuses null pointers, an empty extent, a radius that is not positive and an unknown depth mode
    (status 1), and the StochasticDepth mode (status 2), on the host, before any GPU work; so do
    rsd_hbao_noise_table and rsd_cross_bilateral_blur_src."""
    L = abi.lib()
    cam, prm = abi.Camera(), abi.HBAOParams()
    ok = dict(z=C.c_void_p(1 << 20), z2=C.c_void_p(2 << 20), n=C.c_void_p(3 << 20), w=8, h=8, cam=C.byref(cam),
              prm=prm, out=C.c_void_p(4 << 20))  # never dereferenced: the checks come first

    def call(**kw):
        a = {**ok, **kw}
        return L.rsd_hbao(a["z"], a["z2"], a["n"], a["w"], a["h"], a["cam"],
                          C.byref(a["prm"]) if a["prm"] is not None else None, a["out"], None)

    bad_params = [abi.HBAOParams(radius=0.0), abi.HBAOParams(radius=-1.0), abi.HBAOParams(radius=float("nan")),
                  abi.HBAOParams(depth_mode=3)]
    for bad in [dict(z=None), dict(n=None), dict(cam=None), dict(prm=None), dict(out=None), dict(w=0), dict(h=0),
                dict(prm=abi.HBAOParams(depth_mode=HB.DUAL), z2=None)] + [dict(prm=p) for p in bad_params]:
        assert call(**bad) == abi.ERR_INVALID_ARG, bad
        assert b"rsd_hbao" in L.rsd_last_error(), bad
    assert call(prm=abi.HBAOParams(depth_mode=2)) == abi.ERR_UNSUPPORTED
    assert b"StochasticDepth" in L.rsd_last_error()
    assert call(prm=abi.HBAOParams(depth_mode=2), z2=None) == abi.ERR_UNSUPPORTED
    assert L.rsd_hbao_noise_table(None) == abi.ERR_INVALID_ARG
    p = C.c_void_p(1 << 20)
    for nbytes in (0, 3, 4):
        assert L.rsd_cross_bilateral_blur_src(p, nbytes, p, 8, 8, p, p, 8, 8, 0, 4, 1, None) == abi.ERR_INVALID_ARG
        assert b"src_texel_bytes" in L.rsd_last_error()
    assert L.rsd_cross_bilateral_blur_src(None, 2, p, 8, 8, p, p, 8, 8, 0, 4, 1, None) == abi.ERR_INVALID_ARG
    assert L.rsd_cross_bilateral_blur_src(p, 2, p, 8, 8, p, p, 8, 8, 4, 4, 1, None) == abi.ERR_INVALID_ARG  # guard band


# ---------------------------------------------------------------------------------- the noise table

@needs_gcc
def test_noise_table(checker):
    """rsd_hbao_noise_table is the checker's table bit for bit, and both start with MT19937(0)'s known draws
    (libstdc++'s std::mt19937(0), numpy's RandomState(0)) mapped as u / 2^32."""
    want, first3, theta0 = HB.noise_table(checker)
    assert first3.tolist() == [2357136044, 2546248239, 3071714933]
    assert F(theta0) == F(3.44764662) and want[0, 2] == F(0.592844605) and want[0, 3] == F(0.715189338)
    assert want[0, 0] == F(np.sin(np.float64(F(theta0)))) and want[0, 1] == F(np.cos(np.float64(F(theta0))))
    got = np.zeros((16, 4), F)
    abi.check(abi.lib().rsd_hbao_noise_table(got.ctypes.data_as(C.c_void_p)), "rsd_hbao_noise_table")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    np.testing.assert_allclose(got[:, 0] ** 2 + got[:, 1] ** 2, 1.0, atol=1e-6)
    assert ((got[:, 2:] >= 0) & (got[:, 2:] < 1)).all() and len(np.unique(got[:, 2:])) == 32
    assert np.array_equal(np.array(abi.HBAOParams().rand, F).view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------- checker known answers

def _facing_normals(cam, width, height):
    """World-space normals that the view matrix turns into (0, 0, 1): its third row."""
    n = np.zeros((height, width, 4), F)
    n[..., :3] = np.array(list(cam.viewMat), F).reshape(4, 4)[2, :3]
    return n


@needs_gcc
@pytest.mark.parametrize("mode", [HB.SINGLE, HB.DUAL])
def test_checker_flat_floor_is_unoccluded(checker, mode):
    """A plane of constant depth seen head-on: every tap lies in the pixel's tangent plane, NdotV = 0 falls below
    the bias, nothing occludes: (255, 255) on every texel of every layer, ragged ones included."""
    W, H = 150, 90
    cam = HB.camera(W, H)
    z = HB.deinterleave(np.full((H, W), 5.0, F))
    z[z == 0] = F(5.0)  # the layers' texels beyond the frame
    out, flags = HB.hbao(checker, z, z + F(1.0), _facing_normals(cam, W, H), cam, depth_mode=mode)
    assert (out == 255).all()
    assert (flags & (HB.FAR | HB.SMALL | HB.SCISSORED | HB.NAN_TAP) == 0).all()
    assert HB.shares(flags)["ragged_texels"] == 16 * 38 * 23 - 150 * 90


@needs_gcc
def test_checker_far_plane_and_small_radius_early_outs(checker):
    """linearDepth >= farZ gives (1, 1) whatever surrounds the pixel, and so does a radius below one pixel."""
    W, H = 64, 48
    s = HB.synthetic(W, H)
    cam, far = s["cam"], F(s["cam"].farZ)
    out, flags = HB.hbao(checker, s["layers"], None, s["normal_w"], cam, radius=1.0)
    at_far = HB.deinterleave(s["z"]) >= far
    assert at_far.sum() > 100 and ((flags & HB.FAR) != 0)[at_far].all() and (out[at_far] == 255).all()
    assert not ((flags & HB.FAR) != 0)[~at_far].any()
    assert (out[~at_far] < 255).any()
    just_below = np.where(at_far, np.nextafter(far, F(0)), s["layers"]).astype(F)
    _, flags2 = HB.hbao(checker, just_below, None, s["normal_w"], cam, radius=1.0)
    assert not (flags2 & HB.FAR).any()
    tiny, flags3 = HB.hbao(checker, s["layers"], None, s["normal_w"], cam, radius=1e-4)
    shaded = (s["layers"] > 0) & ~at_far
    assert ((flags3 & HB.SMALL) != 0)[shaded].all() and (tiny[shaded] == 255).all()


@needs_gcc
def test_checker_step_edge_darkens_the_lower_side_only(checker):
    """Two head-on planes, the left one 0.3 nearer: the left (upper) side sees the right one below its tangent
    plane and stays (255, 255); the right (lower) side is darkened next to the edge, in both channels, and not
    beyond the reach of the last step."""
    W, H = 96, 48
    cam = HB.camera(W, H)
    z = np.full((H, W), 4.0, F)
    z[:, W // 2:] = F(4.3)
    out, flags = HB.hbao(checker, HB.deinterleave(z), None, _facing_normals(cam, W, H), cam, radius=1.0)
    assert (flags == 0).all()
    full = HB.interleave(out, W, H)
    assert (full[:, :W // 2] == 255).all()
    assert (full[:, W // 2:W // 2 + 4] < 255).all()
    assert (full[:, W // 2:W // 2 + 4, 0] >= full[:, W // 2:W // 2 + 4, 1]).all()  # the dark channel has no falloff
    # radius in pixels 0.875 * 48 / 4.3 = 9.8: the last tap lies at most 1 + 5 * 9.8 / 20 = 3.4 quarter texels away
    assert (full[:, W // 2 + 16:] == 255).all()


@needs_gcc
def test_checker_dual_depth_only_adds_occlusion(checker):
    """DualDepth takes a per-channel max over the layers, so no texel gets brighter than in SingleDepth; with a
    second layer equal to the first it changes nothing."""
    s = HB.synthetic(64, 48)
    one, _ = HB.hbao(checker, s["layers"], None, s["normal_w"], s["cam"])
    two, flags = HB.hbao(checker, s["layers"], s["layers2"], s["normal_w"], s["cam"], depth_mode=HB.DUAL)
    same, _ = HB.hbao(checker, s["layers"], s["layers"], s["normal_w"], s["cam"], depth_mode=HB.DUAL)
    assert (two <= one).all() and (two < one).any()
    assert np.array_equal(same, one)
    changed = (two != one).any(-1)
    assert (HB.recompute_count(flags)[changed] > 0).all()


@needs_gcc
def test_checker_ragged_frame_keeps_the_two_resolutions(checker):
    """150 x 90: texC uses 1 / (150, 90) while the layers are 38 x 23 texels, so the centre tap of texel x reads
    texel floor((4 x + dx + 0.5) * 38 / 150) of its layer, which for dx = 3 is x + 1 from x = 9 on: with one column of
    the layers at farZ, the far early out shows which texel each centre tap read."""
    W, H = 150, 90
    cam = HB.camera(W, H)
    col = np.broadcast_to(np.arange(38, dtype=F), (16, 23, 38))
    z = np.where(col == 30, F(cam.farZ), F(5.0)).astype(F)  # only column 30 is at farZ
    _, flags = HB.hbao(checker, z, None, _facing_normals(cam, W, H), cam)
    for layer, want in ((0, [30]), (3, [29]), (15, [29])):
        dx = layer % 4
        read = [int(np.floor(F(F(4 * x + dx + 0.5) * (F(1) / F(W))) * F(38))) for x in range(38)]
        assert [x for x in range(38) if read[x] == 30] == want
        assert np.unique(np.nonzero(flags[layer] & HB.FAR)[1]).tolist() == want, layer


@needs_gcc
def test_checker_rounds_ties_to_even(checker):
    """HB.tie_case: every shaded texel has taps exactly between two texels, and the checker sends the tap at 2.5
    quarter texels to texel 2, not 3: with the column written into the depth the far early out cannot tell, so
    the check is on the occlusion -- a wall 2 texels to the right occludes, the same wall 3 texels away does not
    change a byte of the texels whose only tap there is the tie."""
    t = HB.tie_case()
    out, flags = HB.hbao(checker, t["layers"], None, t["normal_w"], t["cam"], radius=t["radius"], rand=t["rand"])
    assert ((flags & HB.TIE) != 0).mean() > 0.95 and (flags & (HB.FAR | HB.SMALL) == 0).all()
    assert len(np.unique(out)) > 20
    # flat depth, so only direction 0 = (1, 0) reaches columns x + 1 .. x + 3, with taps at 1, round(1.5) = 2, 2
    # and round(2.5) = 2: a change of column x + 3 alone leaves texel x's bytes as they are
    x = 6
    wall = np.array(t["layers"])
    wall[:, :, x + 3] = F(3.5)
    out3, _ = HB.hbao(checker, wall, None, t["normal_w"], t["cam"], radius=t["radius"], rand=t["rand"])
    wall = np.array(t["layers"])
    wall[:, :, x + 2] = F(3.5)
    out2, _ = HB.hbao(checker, wall, None, t["normal_w"], t["cam"], radius=t["radius"], rand=t["rand"])
    assert np.array_equal(out3[:, :, x], out[:, :, x])
    assert (out2[:, :, x] != out[:, :, x]).any()


# ---------------------------------------------------------------------------------- input conditions

@needs_gcc
@pytest.mark.parametrize("size", HB.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_inputs_reach_every_path(checker, size):
    """The synthetic input of the GPU parity test at this size reaches every path of the shader, on the checker
    alone: at the middle radius far, small-radius and shaded texels each hold >= 2 %; in DualDepth RecomputeAO
    fires on >= 5 % of the shaded texels and changes a byte against SingleDepth on at least one of them; a texel
    has a NaN tap; at guard band 8 the scissored count is the one the sizes give; and the three radii leave the
    small-radius early out none, some and most of the texels."""
    W, H = size
    s = HB.synthetic(W, H)
    r_all, r_mid, r_small = HB.radii(H)
    run = lambda **kw: HB.hbao(checker, s["layers"], s["layers2"], s["normal_w"], s["cam"], **kw)  # noqa: E731
    for guard in HB.GUARDS:
        one, f1 = run(radius=r_mid, guard_band=guard)
        two, f2 = run(radius=r_mid, guard_band=guard, depth_mode=HB.DUAL)
        sh1, sh2 = HB.shares(f1), HB.shares(f2)
        print(W, H, "guard", guard, sh1, "dual recompute", sh2["recompute_of_shaded"])
        for k in ("far", "small", "shaded"):
            assert sh1[k] >= 0.02 and sh2[k] == sh1[k], (k, sh1, sh2)
        assert sh1["recompute_of_shaded"] == 0.0 and sh2["recompute_of_shaded"] >= 0.05, sh2
        inside = (f2 & HB.SCISSORED) == 0
        fired = (HB.recompute_count(f2) > 0) & inside
        assert ((two != one).any(-1) & fired).sum() >= 1
        assert not ((two != one).any(-1) & ~fired).any()
        nan_inside = ((f1 & HB.NAN_TAP) != 0) & inside
        assert nan_inside.sum() >= 1, sh1
        assert sh1["scissored_texels"] == HB.scissored_texels(W, H, guard)
        assert (one[~inside] == HB.SENTINEL).all() and inside.sum() == 16 * f1[0].size - sh1["scissored_texels"]
        assert sh1["ragged_texels"] == 16 * f1[0].size - W * H
    assert HB.scissored_texels(W, H, 0) == 0 and HB.scissored_texels(W, H, 8) > 0
    small = [HB.shares(run(radius=r)[1])["small"] for r in (r_all, r_mid, r_small)]
    print(W, H, "small-radius share at the three radii", small)
    assert small[0] == 0.0 and 0.02 <= small[1] <= 0.6 and small[2] >= 0.6, small
    for exponent in HB.EXPONENTS:  # both exponents give intermediate values in both channels
        out, _ = run(radius=r_all, exponent=exponent)
        for ch in range(2):
            assert len(np.unique(out[..., ch])) > 50, (exponent, ch)
    a, b = run(radius=r_all, exponent=2.0)[0], run(radius=r_all, exponent=1.7)[0]
    assert (a != b).mean() > 0.1
    # no answer at any parameter point of the GPU parity test is the sentinel pair, so a sentinel left inside the
    # scissor there can only be a texel that was not written
    for mode in (HB.SINGLE, HB.DUAL):
        for guard in HB.GUARDS:
            for radius in HB.radii(H):
                for exponent in HB.EXPONENTS:
                    out, f = run(radius=radius, exponent=exponent, depth_mode=mode, guard_band=guard)
                    inside = (f & HB.SCISSORED) == 0
                    assert not (out[inside] == HB.SENTINEL).all(-1).any(), (mode, guard, radius, exponent)
