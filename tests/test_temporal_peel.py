"""CPU checks of the TemporalDepthPeel feature (rsd_temporal_depth_peel, the TemporalDepthPeel graph pass):
the pass is registered and reflects like the reference's, our DualDepth graph script and the reference's
SVAO_depth.py plan with it, the C entry refuses bad arguments without a GPU, the scalar checker the GPU tests
compare against (tests/native/temporal_peel_ref.c) gives the answers that can be known in advance, and the
inputs of the GPU tests reach every part of the shader (asserted on the checker alone)."""
import ctypes as C
import shutil
from pathlib import Path

import numpy as np
import pytest

import temporal_peel_checker as TP
from conftest import ROOT

rsdgraph = pytest.importorskip("rsd.graph")
from rsd import abi  # noqa: E402

SCRIPT = ROOT / "tests" / "graphs" / "svao_dual_temporal.py"
REF_SCRIPTS = Path("/root/reference/scripts")
needs_gcc = pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
F = np.float32


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return TP.build(tmp_path_factory.mktemp("temporal_peel_ref"))


def test_temporal_depth_peel_is_a_builtin_pass():
    assert "TemporalDepthPeel" in rsdgraph.plugin_types()


def test_reflection():
    """TemporalDepthPeel::reflect (:137-146): linearZ and mvec in, depth2 (R32Float) out; the producers
    (stubs) take the declared input formats."""
    g = rsdgraph.RenderGraph("tdp")
    g.create_pass("T", "TemporalDepthPeel", {})
    g.create_pass("Z", "Source", {})
    g.create_pass("M", "Source", {})
    g.add_edge("Z.z", "T.linearZ")
    g.add_edge("M.mv", "T.mvec")
    g.mark_output("T.depth2")
    g.plan(100, 60)
    res = g.resources()
    assert res["T.depth2"] == (100, 60, 1, "R32Float")
    assert res["Z.z"][3] == "R32Float" and res["M.mv"][3] == "RG32Float"
    # both inputs are required: without the mvec edge the graph does not plan
    g = rsdgraph.RenderGraph("tdp2")
    g.create_pass("T", "TemporalDepthPeel", {})
    g.create_pass("Z", "Source", {})
    g.add_edge("Z.z", "T.linearZ")
    g.mark_output("T.depth2")
    with pytest.raises(abi.RsdError, match="T.mvec"):
        g.plan(100, 60)
    # an unknown property warns and the pass is still created, like the reference's
    g.create_pass("U", "TemporalDepthPeel", {"minSeparationDistance": 0.05, "someFutureKey": 1})


def test_dual_temporal_script_plans():
    g = rsdgraph.load_script(SCRIPT)["SVAODualTemporal"]
    g.plan(192, 128)
    order = g.execution_order()
    chain = ["GBufferRaster", "LinearizeDepth", "TemporalDepthPeel", "DepthSelect", "SVAO"]
    assert [order.index(p) for p in chain] == sorted(order.index(p) for p in chain), order
    res = g.resources()
    assert res["TemporalDepthPeel.depth2"] == (192, 128, 1, "R32Float")
    assert res["DepthSelect.out"] == (192, 128, 1, "R32Float")
    assert res["GBufferRaster.mvec"] == (192, 128, 1, "RG32Float")


@pytest.mark.skipif(not REF_SCRIPTS.is_dir(), reason="reference scripts not present (GPU box)")
def test_reference_script_plans_with_the_real_pass():
    g = next(iter(rsdgraph.load_script(REF_SCRIPTS / "SVAO_depth.py").values()))
    g.plan(1920 + 128, 1080 + 128)
    order = g.execution_order()
    assert order.index("LinearizeDepth") < order.index("TemporalDepthPeel") < order.index("DepthSelect") < \
        order.index("SVAO")
    assert g.resources()["TemporalDepthPeel.depth2"] == (2048, 1208, 1, "R32Float")


def test_arguments_are_checked():
    """rsd_temporal_depth_peel refuses every null argument, an empty extent, max_iterations outside 0..256 and
    an output that aliases the history, on the host (status 1, a message naming the function), before any
    GPU work."""
    L = abi.lib()
    cam = abi.Camera()
    m = (C.c_float * 16)()
    ok = dict(z=C.c_void_p(1 << 20), prev=C.c_void_p(2 << 20), w=8, h=8, cam=C.byref(cam), c2p=m, p2c=m, it=32,
              out=C.c_void_p(3 << 20))  # never dereferenced: the checks come first

    def call(**kw):
        a = {**ok, **kw}
        return L.rsd_temporal_depth_peel(a["z"], a["prev"], a["w"], a["h"], a["cam"], a["c2p"], a["p2c"], 0.5,
                                         a["it"], a["out"], None)

    for bad in (dict(z=None), dict(prev=None), dict(cam=None), dict(c2p=None), dict(p2c=None), dict(out=None),
                dict(w=0), dict(h=0), dict(it=-1), dict(it=257), dict(out=ok["prev"]),
                dict(out=C.c_void_p((2 << 20) + 4 * 63))):  # the last texel of the history
        assert call(**bad) == abi.ERR_INVALID_ARG, bad
        assert b"rsd_temporal_depth_peel" in L.rsd_last_error(), bad


def test_view_matrices():
    """cur_view_to_prev_view is the inverse of prev_view_to_cur_view, and is it with the cameras swapped; a
    camera that moved along +x sees a previous-view point further along -x."""
    from rsd.frame import FrameConfig, look_at
    from rsd.temporal import cur_view_to_prev_view, prev_view_to_cur_view
    cfg = FrameConfig(visible_w=64, visible_h=64, guard_band=0)
    prev = look_at([0.0, 2.0, 8.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0], cfg)
    cur = look_at([0.5, 2.1, 7.7], [0.3, 1.0, 0.0], [0.0, 1.0, 0.0], cfg)
    c2p, p2c = cur_view_to_prev_view(cur, prev), prev_view_to_cur_view(cur, prev)
    assert c2p.dtype == np.float32 and c2p.shape == (4, 4)
    np.testing.assert_allclose(c2p.astype(np.float64) @ p2c.astype(np.float64), np.eye(4), atol=1e-5)
    assert np.array_equal(c2p, prev_view_to_cur_view(prev, cur))
    shifted = look_at([1.0, 2.0, 8.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0], cfg)  # prev moved by +1 in x (view x too)
    np.testing.assert_allclose(prev_view_to_cur_view(shifted, prev)[:3, 3], [-1.0, 0.0, 0.0], atol=1e-5)
    np.testing.assert_allclose(cur_view_to_prev_view(shifted, prev)[:3, 3], [1.0, 0.0, 0.0], atol=1e-5)


# ---------------------------------------------------------------------------------- checker known answers

def _identity_case(width=40, height=30):
    from rsd.frame import FrameConfig, look_at
    cam = look_at([0.0, 2.0, 8.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0], FrameConfig(visible_w=width, visible_h=height,
                                                                                  guard_band=0))
    rng = np.random.default_rng(3)
    z = (2.0 + 0.25 * rng.integers(0, 41, (height, width))).astype(F)  # multiples of 0.25: no near ties below
    return cam, z, np.eye(4, dtype=F)


@needs_gcc
def test_checker_zero_history_returns_the_first_layer(checker):
    cam, z, eye = _identity_case()
    s = TP.synthetic(checker, 75, 45, "turn")
    for zz, c2p, p2c, c in ((z, eye, eye, cam), (s["z"], s["c2p"], s["p2c"], s["cam"])):
        for sep in TP.SEPARATIONS:
            out, flags = TP.peel(checker, zz, np.zeros_like(zz), c, c2p, p2c, sep, 32)
            assert np.array_equal(TP.bits(out), TP.bits(zz))
            assert ((flags & TP.BEST_ZERO) != 0).all()


@needs_gcc
def test_checker_constant_history_under_identity(checker):
    """Identity matrices and a previous map of one constant c: the ray is a point, its one sample a zlerp of four
    equal texels (c to a few ulp), the way back an identity.  Interior pixels with depth + sep < c < 0.99 farZ give c
    within 1e-6 relative; every other pixel gives its depth (the border rows and columns, whose footprint holds
    border texels, included)."""
    cam, z, eye = _identity_case()
    H, W = z.shape
    c, sep = F(9.1), F(0.5)
    out, flags = TP.peel(checker, z, np.full_like(z, c), cam, eye, eye, sep, 32)
    interior = np.zeros_like(z, bool)
    interior[1:-1, 1:-1] = True
    hit = interior & (z + sep < c)
    assert hit.sum() > 0.3 * z.size and (~hit & interior).sum() > 0.1 * z.size
    assert (np.abs(out[hit] - c) <= 1e-6 * c).all()
    assert np.array_equal(TP.bits(out[~hit & interior]), TP.bits(z[~hit & interior]))
    border_ok = np.isclose(out[~interior], c, rtol=1e-6) | (TP.bits(out[~interior]) == TP.bits(z[~interior]))
    assert border_ok.all()
    assert ((flags & TP.EXIT_MASK) == TP.EXIT_UV).all()  # a zero-length interval ends the search at once
    # a constant above 0.99 farZ is never written
    far = F(cam.farZ)
    out, flags = TP.peel(checker, z, np.full_like(z, F(0.995) * far), cam, eye, eye, sep, 32)
    assert np.array_equal(TP.bits(out), TP.bits(z))
    assert ((flags & TP.POINT) != 0)[interior].all()


@needs_gcc
def test_checker_separation_test_is_strict(checker):
    """A sample that comes back exactly at depth + min_separation is not written (`>`, ps.slang:311 and :422); one
    that comes back an ulp behind it is.  TP.boundary_case holds both kinds."""
    cam, z, hist, eye = TP.boundary_case()
    out, flags = TP.peel(checker, z, hist, cam, eye, eye, 0.5, 32)
    on = (flags & TP.ON_BOUND) != 0
    written = TP.bits(out) != TP.bits(z)
    print("on the bound:", int(on.sum()), "written:", int(written.sum()), "of", z.size)
    assert on.sum() >= 10 and written.sum() >= 10
    assert not (on & written).any()
    assert (out[written] > z[written] + F(0.5)).all() and (out[written] < F(4.50001)).all()


@needs_gcc
def test_checker_zero_iterations_returns_the_first_layer(checker):
    s = TP.synthetic(checker, 75, 45, "step")
    out, flags = TP.peel(checker, s["z"], s["prev2"], s["cam"], s["c2p"], s["p2c"], 0.5, 0)
    assert np.array_equal(TP.bits(out), TP.bits(s["z"]))
    assert ((flags & TP.EXIT_MASK) == TP.EXIT_ITER).all()


# ---------------------------------------------------------------------------------- input conditions

@needs_gcc
@pytest.mark.parametrize("size", TP.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_inputs_reach_every_class(checker, size):
    """The synthetic input of the GPU parity test at this size (one linearZ / history pair seen from the two
    previous poses, run over the 3 x 3 grid of min_separation and max_iterations) reaches every class of
    pixels, on the checker alone.

    Which run can reach which class follows from the shader: with max_iterations = 32 the uv interval always
    falls below half a texel before the iterations run out, so only the runs with 1 and 7 iterations end
    on the iteration count; min_separation = 0 makes the `< minSeparationDist * 0.001` exit impossible, and noise
    never comes that close, so that exit is reached on the flat patch at the separation it was placed for (0.5);
    rays leave the previous screen for the "turn" pose.  So each class must reach its share in at least one run
    of the input, while every run must write both kinds of pixel on >= 10 % and never hit the clip cap."""
    W, H = size
    best = {}
    for pose in TP.POSES:
        s = TP.synthetic(checker, W, H, pose)
        for sep in TP.SEPARATIONS:
            for it in TP.ITERATIONS:
                out, flags = TP.peel(checker, s["z"], s["prev2"], s["cam"], s["c2p"], s["p2c"], sep, it)
                sh = TP.shares(flags, out, s["z"])
                print(W, H, pose, sep, it, sh)
                assert not np.isnan(out).any()
                assert sh["clip_cap_px"] == 0
                assert sh["moved"] >= 0.10 and sh["kept"] >= 0.10, (pose, sep, it, sh)
                for k, v in sh.items():
                    best[k] = max(best.get(k, 0), v)
    assert best["exit_uv"] >= 0.01 and best["exit_z"] >= 0.01 and best["exit_iter"] >= 0.01, best
    assert best["clipped"] >= 0.05, best
    assert best["point"] >= 0.01, best
    assert best["quirk0_px"] >= 1, best


@needs_gcc
def test_rendered_sequence_finds_a_second_layer(oracle, checker):
    """The 4-pose arcade_tiny sequence of the GPU feedback test, on the oracle's G-buffer and the checker alone:
    frame 0 is the first layer, and the last frame holds a second layer on >= 2 % of its pixels."""
    from helpers import small_frame_config, to_oracle
    from rsd.frame import look_at
    from rsd.scenes import make_scene
    from rsd.temporal import cur_view_to_prev_view, prev_view_to_cur_view
    cfg = small_frame_config()
    scene = make_scene("arcade_tiny")
    osc = oracle.Scene(scene.positions, scene.indices, scene.flags)
    prev_cam, prev2 = None, None
    for i, (pos, tgt, up) in enumerate(TP.sequence_poses(scene)):
        cam = look_at(pos, tgt, up, cfg)
        z = oracle.gbuffer(osc, to_oracle(cam, oracle.Camera), cfg.fb_w, cfg.fb_h, cfg.cull_mode)[0]
        prev_cam = prev_cam or cam
        prev2 = np.zeros_like(z) if prev2 is None else prev2
        out, flags = TP.peel(checker, z, prev2, cam, cur_view_to_prev_view(cam, prev_cam),
                             prev_view_to_cur_view(cam, prev_cam), 0.5, 32)
        share = float((TP.bits(out) != TP.bits(z)).mean())
        print("frame", i, "second layer on", share)
        if i == 0:
            assert share == 0.0
        assert (flags & TP.CLIP_CAP == 0).all()
        prev_cam, prev2 = cam, out
    assert share >= 0.02
