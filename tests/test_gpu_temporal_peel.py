"""GPU: rsd_temporal_depth_peel, the TemporalDepthPeel class and the TemporalDepthPeel graph pass against the
scalar CPU checker (tests/native/temporal_peel_ref.c, whose known answers and input conditions
tests/test_temporal_peel.py asserts).  Every comparison is on float bit patterns."""
import ctypes as C

import numpy as np
import pytest

import temporal_peel_checker as TP
from conftest import ROOT
from helpers import small_frame_config

pytestmark = pytest.mark.gpu
F = np.float32
SCRIPT = ROOT / "tests" / "graphs" / "svao_dual_temporal.py"
PEEL_SCRIPT = ROOT / "tests" / "graphs" / "svao_dual_peel.py"


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return TP.build(tmp_path_factory.mktemp("temporal_peel_ref"))


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def inputs(checker):
    """The synthetic inputs, built once and shared (read-only) by every parameter point."""
    out = {}
    for size in TP.SIZES:
        for pose in TP.POSES:
            s = TP.synthetic(checker, *size, pose)
            for a in (s["z"], s["prev2"]):
                a.setflags(write=False)
            out[size, pose] = s
    return out


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("iterations", TP.ITERATIONS)
@pytest.mark.parametrize("sep", TP.SEPARATIONS)
@pytest.mark.parametrize("pose", TP.POSES)
@pytest.mark.parametrize("size", TP.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_parity(torch, checker, inputs, size, pose, sep, iterations):
    """rsd_temporal_depth_peel equals the checker bit for bit, and writes every pixel of a sentinel-filled
    output."""
    from rsd import abi
    s = inputs[size, pose]
    W, H = size
    z, prev = torch.from_numpy(np.array(s["z"])).cuda(), torch.from_numpy(np.array(s["prev2"])).cuda()
    out = torch.full((H, W), float(TP.SENTINEL), dtype=torch.float32, device="cuda")
    c2p, p2c = np.ascontiguousarray(s["c2p"], F), np.ascontiguousarray(s["p2c"], F)
    abi.check(abi.lib().rsd_temporal_depth_peel(_p(z), _p(prev), W, H, C.byref(s["cam"]),
                                                c2p.ctypes.data_as(C.c_void_p), p2c.ctypes.data_as(C.c_void_p),
                                                sep, iterations, _p(out),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "rsd_temporal_depth_peel")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want, flags = TP.peel(checker, s["z"], s["prev2"], s["cam"], c2p, p2c, sep, iterations)
    assert (flags & TP.CLIP_CAP == 0).all()
    assert (got != TP.SENTINEL).all()
    diff = TP.bits(got) != TP.bits(want)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5], got[diff][:5], want[diff][:5])
    assert np.array_equal(prev.cpu().numpy(), s["prev2"]) and np.array_equal(z.cpu().numpy(), s["z"])  # inputs untouched


def test_separation_test_is_strict(torch, checker):
    """Samples exactly at depth + min_separation are not written, samples an ulp behind it are (TP.boundary_case
    holds both, which tests/test_temporal_peel.py asserts on the checker)."""
    from rsd import abi
    cam, z, hist, eye = TP.boundary_case()
    H, W = z.shape
    out = torch.full((H, W), float(TP.SENTINEL), dtype=torch.float32, device="cuda")
    m = eye.ctypes.data_as(C.c_void_p)
    zt, ht = torch.from_numpy(z).cuda(), torch.from_numpy(hist).cuda()
    abi.check(abi.lib().rsd_temporal_depth_peel(_p(zt), _p(ht), W, H, C.byref(cam), m, m, 0.5, 32, _p(out),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "rsd_temporal_depth_peel")
    torch.cuda.synchronize()
    want, flags = TP.peel(checker, z, hist, cam, eye, eye, 0.5, 32)
    assert ((flags & TP.ON_BOUND) != 0).sum() >= 10
    assert np.array_equal(TP.bits(out.cpu().numpy()), TP.bits(want))


@pytest.fixture(scope="module")
def arcade(torch):
    from rsd.frame import Device, GpuScene
    from rsd.scenes import make_scene
    scene = make_scene("arcade_tiny")
    dev = Device(0)
    gs = GpuScene(dev, scene)
    yield dict(scene=scene, dev=dev, gs=gs)
    gs.release()
    dev.close()


def test_first_frame_and_feedback(torch, checker, arcade):
    """The TemporalDepthPeel class over the 4-pose arcade_tiny sequence, linearZ from Renderer's G-buffer: frame 0
    is linearZ, every frame equals the checker chained on its own previous output, the history is the previous
    output, reset() restores frame-0 behaviour and a size change reallocates."""
    from rsd.frame import Renderer
    from rsd.temporal import TemporalDepthPeel, cur_view_to_prev_view, prev_view_to_cur_view
    scene = arcade["scene"]
    cfg = small_frame_config()
    r = Renderer(scene, cfg, gpu_scene=arcade["gs"], dev=arcade["dev"])
    tdp = TemporalDepthPeel()
    assert (tdp.min_separation, tdp.iterations) == (0.5, 32)
    prev_cam, want_prev = None, None
    for i, pose in enumerate(TP.sequence_poses(scene)):
        r.set_pose(*pose)
        r.gbuffer()
        prev_cam = prev_cam or r.cam
        out = torch.full_like(r.depth, float(TP.SENTINEL))
        assert tdp.execute(r.depth, r.cam, prev_cam, depth2_out=out) is out
        torch.cuda.synchronize()
        z, got = r.depth.cpu().numpy(), out.cpu().numpy()
        want_prev = np.zeros_like(z) if want_prev is None else want_prev
        want, _ = TP.peel(checker, z, want_prev, r.cam, cur_view_to_prev_view(r.cam, prev_cam),
                          prev_view_to_cur_view(r.cam, prev_cam), 0.5, 32)
        assert np.array_equal(TP.bits(got), TP.bits(want)), i
        if i == 0:
            assert np.array_equal(TP.bits(got), TP.bits(z))
        assert np.array_equal(TP.bits(tdp.prev_depth2.cpu().numpy()), TP.bits(got)), i  # the history is this output
        assert tdp.prev_depth2.data_ptr() != out.data_ptr()
        prev_cam, want_prev = r.cam, want
    moved = (TP.bits(got) != TP.bits(z)).mean()
    assert moved >= 0.02, moved
    # reset(): the same frame again, now without a history, is the first layer
    tdp.reset()
    again = tdp.execute(r.depth, r.cam, prev_cam)
    torch.cuda.synchronize()
    assert np.array_equal(TP.bits(again.cpu().numpy()), TP.bits(z))
    # ... and with that history (the first layer of the same pose) it is the checker's answer for it
    twice = tdp.execute(r.depth, r.cam, r.cam).cpu().numpy()
    eye_c2p, eye_p2c = cur_view_to_prev_view(r.cam, r.cam), prev_view_to_cur_view(r.cam, r.cam)
    assert np.array_equal(TP.bits(twice), TP.bits(TP.peel(checker, z, z, r.cam, eye_c2p, eye_p2c, 0.5, 32)[0]))
    # a size change reallocates a zeroed history
    small = r.depth[:40, :60].contiguous()
    first = tdp.execute(small, r.cam, r.cam)
    torch.cuda.synchronize()
    assert tuple(tdp.prev_depth2.shape) == (40, 60)
    assert np.array_equal(TP.bits(first.cpu().numpy()), TP.bits(small.cpu().numpy()))
    with pytest.raises(ValueError):
        tdp.execute(r.depth.double(), r.cam, r.cam)


def _np(t):
    return t.cpu().numpy()


def test_graph_dual_depth_from_temporal_depth_peel(torch, arcade):
    """tests/graphs/svao_dual_temporal.py executed for 3 frames with a moving camera: TemporalDepthPeel.depth2 is
    the class's output on the graph's own linear depth, DepthSelect forwards it, and SVAO (DualDepth, exact
    numerics) equals a direct DualDepth Renderer frame given the same G-buffer and depth2.  With selected = 1
    the graph still equals the DepthPeeling chain."""
    from rsd import abi
    from rsd import graph as rg
    from rsd.frame import Renderer, look_at
    from rsd.temporal import TemporalDepthPeel
    scene, gs = arcade["scene"], arcade["gs"]
    cfg = small_frame_config()
    cfg.primary, cfg.numerics = abi.DEPTH_DUAL, "exact"
    H, W = cfg.fb_h, cfg.fb_w
    r = Renderer(scene, cfg, gpu_scene=gs, dev=arcade["dev"])
    poses = TP.sequence_poses(scene, 3)

    def direct(cam, z, normals, depth2):
        r.cam = cam
        r.depth.copy_(z.reshape(H, W))
        r.normals.copy_(normals.reshape(H, W).view(torch.int16))
        r.depth2.copy_(depth2.reshape(H, W))
        r.ao.zero_()
        r.frame()
        torch.cuda.synchronize()
        return _np(r.ao)

    g = rg.load_script(SCRIPT)["SVAODualTemporal"]
    tdp = TemporalDepthPeel(0.5)
    prev_cam, moved = None, 0.0
    for i, pose in enumerate(poses):
        cam = look_at(*pose, cfg)
        g.set_scene(gs.h, cam)
        if i == 0:
            g.compile(W, H)
        g.execute()
        torch.cuda.synchronize()
        z = g.output_tensor("LinearizeDepth.linearDepth").reshape(H, W).contiguous()
        d2 = g.output_tensor("TemporalDepthPeel.depth2").reshape(H, W)
        want = tdp.execute(z, cam, prev_cam or cam)
        torch.cuda.synchronize()
        assert np.array_equal(TP.bits(_np(d2)), TP.bits(_np(want))), i
        assert np.array_equal(TP.bits(_np(g.output_tensor("DepthSelect.out")).reshape(H, W)), TP.bits(_np(d2))), i
        ao = _np(g.output_tensor("SVAO.ao")).reshape(H, W)
        assert np.array_equal(ao, direct(cam, z, g.output_tensor("CompressNormals.normalOut"), d2)), i
        moved = float((TP.bits(_np(d2)) != TP.bits(_np(z))).mean())
        prev_cam = cam
    assert moved >= 0.02, moved  # the last frame's second layer is not just the first
    g.close()

    # selected = 1: the DepthPeeling chain, as before this pass existed
    text = SCRIPT.read_text()
    assert "'selected': 0" in text
    g1 = rg.load_script(text.replace("'selected': 0", "'selected': 1"))["SVAODualTemporal"]
    peel_text = PEEL_SCRIPT.read_text()
    for a, b in (("'guardBand': 8", "'guardBand': 16"), ("'radius': 2.0", "'radius': 1.0"),
                 ("'stochMapDivisor': 1", "'stochMapDivisor': 2"), ("'stochGuardBand': 16", "'stochGuardBand': 64")):
        assert a in peel_text
        peel_text = peel_text.replace(a, b)
    gp = rg.load_script(peel_text)["SVAODualPeel"]
    cam = look_at(*poses[1], cfg)
    for gr in (g1, gp):
        gr.set_scene(gs.h, cam)
        gr.compile(W, H)
        gr.execute()
    torch.cuda.synchronize()
    peeled = _np(gp.output_tensor("LinearizeDepth0.linearDepth"))
    assert np.array_equal(TP.bits(_np(g1.output_tensor("DepthSelect.out"))), TP.bits(peeled))
    assert np.array_equal(TP.bits(_np(g1.output_tensor("LinearizeDepth2Ref.linearDepth"))), TP.bits(peeled))
    assert np.array_equal(_np(g1.output_tensor("SVAO.ao")), _np(gp.output_tensor("SVAO.ao")))
    assert (peeled < cam.farZ).mean() > 0.02
    g1.close()
    gp.close()
