"""GPU: rsd_depth_peel, the DepthPeeling graph pass and Renderer.depth_peel against the brute-force CPU
checker (tests/native/depth_peel_ref.c, pinned to the oracle by tests/test_depth_peel.py).  Every
comparison is bitwise.  75 x 45 frames of ~3000-triangle scenes: partial 8 x 8 tiles on both axes."""
import ctypes as C

import numpy as np
import pytest

import depth_peel_checker as DP
from conftest import ROOT
from helpers import to_oracle

pytestmark = pytest.mark.gpu

W, H = DP.W, DP.H
SCRIPT = ROOT / "tests" / "graphs" / "svao_dual_peel.py"


@pytest.fixture(scope="session")
def checker(oracle, tmp_path_factory):
    return DP.build(oracle, tmp_path_factory.mktemp("depth_peel_ref"))


class Gpu:
    """The two small scenes on the GPU, with their plain G-buffers (computed once, never modified)."""

    def __init__(self, oracle):
        import torch
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from rsd import abi
        from rsd.frame import Device, GpuScene
        self.torch, self.abi = torch, abi
        self.dev = Device(0)
        self.cases = {k: DP.Case(oracle, k) for k in DP.SCENES}
        self.scenes = {k: GpuScene(self.dev, c.scene) for k, c in self.cases.items()}
        self._gb = {}

    def tensor(self, a):
        return self.torch.from_numpy(np.array(a, np.float32)).cuda()  # a copy: cached inputs are read-only

    def gbuffer(self, kind, cull, raster):
        """Linear depth of rsd_gbuffer (raster=False), or of rsd_gbuffer_raster -> rsd_linearize_depth."""
        key = (kind, cull, raster)
        if key not in self._gb:
            t, abi, c = self.torch, self.abi, self.cases[kind]
            z = t.empty((H, W), dtype=t.float32, device="cuda")
            p = lambda x: C.c_void_p(x.data_ptr())
            if raster:
                d = t.empty((H, W), dtype=t.float32, device="cuda")
                nw = t.empty((H, W, 4), dtype=t.float32, device="cuda")
                abi.check(abi.lib().rsd_gbuffer_raster(self.scenes[kind].h, C.byref(c.cam), W, H, cull, p(d), p(nw),
                                                       None), "rsd_gbuffer_raster")
                abi.check(abi.lib().rsd_linearize_depth(p(d), p(z), W * H, c.cam.nearZ, c.cam.farZ, None),
                          "rsd_linearize_depth")
            else:
                n = t.empty((H, W), dtype=t.int16, device="cuda")
                abi.check(abi.lib().rsd_gbuffer(self.scenes[kind].h, C.byref(c.cam), W, H, cull, p(z), p(n), None),
                          "rsd_gbuffer")
            t.cuda.synchronize()
            arr = z.cpu().numpy()
            arr.setflags(write=False)
            self._gb[key] = arr
        return self._gb[key]

    def peel(self, kind, cull, prev, sep, linear_out, scene=None):
        t, abi = self.torch, self.abi
        pv = self.tensor(prev)
        out = t.full((H, W), -7.0, dtype=t.float32, device="cuda")
        h = scene.h if scene is not None else self.scenes[kind].h
        abi.check(abi.lib().rsd_depth_peel(h, C.byref(self.cases[kind].cam), W, H, cull, C.c_void_p(pv.data_ptr()),
                                           float(sep), int(linear_out), C.c_void_p(out.data_ptr()), None),
                  "rsd_depth_peel")
        t.cuda.synchronize()
        return out.cpu().numpy()

    def close(self):
        for s in self.scenes.values():
            s.release()
        self.dev.close()


@pytest.fixture(scope="module")
def gpu(oracle):
    g = Gpu(oracle)
    yield g
    g.close()


@pytest.fixture(scope="module")
def layer2(oracle, checker, gpu):
    """Test 2's inputs and result: prev = rsd_gbuffer's depth, Back cull, separation 0.5, linear output."""
    prev = gpu.gbuffer("opaque", 1, raster=False)
    got = gpu.peel("opaque", 1, prev, 0.5, 1)
    want = DP.peel(oracle, checker, gpu.cases["opaque"], 1, prev, 0.5, 1)
    return dict(prev=prev, got=got, want=want)


@pytest.mark.parametrize("sep", [0.01, 0.5])
@pytest.mark.parametrize("cull", [0, 1, 2])
def test_raster_output_matches_the_checker(oracle, checker, gpu, cull, sep):
    """prev = the linearised rsd_gbuffer_raster depth, what the graph feeds the pass."""
    prev = gpu.gbuffer("opaque", cull, raster=True)
    got = gpu.peel("opaque", cull, prev, sep, 0)
    want = DP.peel(oracle, checker, gpu.cases["opaque"], cull, prev, sep, 0)
    np.testing.assert_array_equal(DP.bits(got), DP.bits(want))
    assert (want < 1.0).any() and (want == 1.0).any()


def test_linear_output_matches_the_checker(gpu, layer2):
    far = np.float32(gpu.cases["opaque"].cam.farZ)
    np.testing.assert_array_equal(DP.bits(layer2["got"]), DP.bits(layer2["want"]))
    n2 = int((layer2["got"] < far).sum())
    assert n2 >= 0.05 * W * H and int((layer2["got"] == far).sum()) >= 0.05 * W * H
    assert n2 + int((layer2["got"] == far).sum()) == W * H  # every cleared pixel is exactly farZ


def test_predicate_is_strict_at_the_boundary(oracle, checker, gpu, layer2):
    """A hit exactly at prev + 0 is discarded; one ulp behind prev it is kept.  The traversal's lower bound
    must not decide either."""
    c = gpu.cases["opaque"]
    far = np.float32(c.cam.farZ)
    z2 = layer2["got"]
    has = z2 < far
    third = gpu.peel("opaque", 1, z2, 0.0, 1)
    assert not (DP.bits(third)[has] == DP.bits(z2)[has]).any()
    assert (third[has] > z2[has]).all()
    np.testing.assert_array_equal(DP.bits(third), DP.bits(DP.peel(oracle, checker, c, 1, z2, 0.0, 1)))
    before = np.nextafter(z2, np.float32(0.0), dtype=np.float32)
    again = gpu.peel("opaque", 1, before, 0.0, 1)
    np.testing.assert_array_equal(DP.bits(again)[has], DP.bits(z2)[has])
    np.testing.assert_array_equal(DP.bits(again), DP.bits(DP.peel(oracle, checker, c, 1, before, 0.0, 1)))


def test_special_prev_values(oracle, checker, gpu):
    """NaN, +inf, farZ, 0 and -1 scattered over the frame: NaN and <= 0 thresholds discard nothing (the
    plain G-buffer depth), +inf discards everything."""
    c = gpu.cases["opaque"]
    far = np.float32(c.cam.farZ)
    plain = gpu.gbuffer("opaque", 1, raster=False)
    vals = np.array([np.nan, np.inf, far, 0.0, -1.0], np.float32)
    which = np.random.default_rng(7).integers(0, len(vals) + 1, size=(H, W))  # len(vals): keep the plain depth
    prev = np.where(which < len(vals), vals[np.minimum(which, len(vals) - 1)], plain).astype(np.float32)
    got = gpu.peel("opaque", 1, prev, 0.0, 1)
    np.testing.assert_array_equal(DP.bits(got), DP.bits(DP.peel(oracle, checker, c, 1, prev, 0.0, 1)))
    first = (which == 0) | (which == 3) | (which == 4)
    np.testing.assert_array_equal(DP.bits(got)[first], DP.bits(plain)[first])
    assert (got[which == 1] == far).all() and (got[which == 2] == far).all()
    assert (plain[first] < far).any()


def test_alpha_scene_matches_the_checker(oracle, checker, gpu):
    """The peeled layer seen through failed alpha texels (alpha test at LOD 0)."""
    c = gpu.cases["alpha"]
    prev = gpu.gbuffer("alpha", 1, raster=False)
    for sep in (0.01, 0.5):
        got = gpu.peel("alpha", 1, prev, sep, 1)
        np.testing.assert_array_equal(DP.bits(got), DP.bits(DP.peel(oracle, checker, c, 1, prev, sep, 1)))
    # the alpha test matters on this frame: with the cards opaque the layer differs
    solid = DP.Case.__new__(DP.Case)
    solid.osc, solid.ocam, solid.has_alpha = c.osc, c.ocam, False
    assert (DP.bits(DP.peel(oracle, checker, solid, 1, prev, 0.5, 1)) != DP.bits(got)).any()


def test_scene_without_triangles_is_all_cleared(gpu):
    from rsd.frame import GpuScene
    from rsd.scenes import Scene
    empty = Scene("empty", np.zeros((1, 3), np.float32), np.zeros((0, 3), np.uint32), np.zeros(0, np.uint32),
                  gpu.cases["opaque"].scene.camera)
    gs = GpuScene(gpu.dev, empty)
    prev = np.zeros((H, W), np.float32)
    far = np.float32(gpu.cases["opaque"].cam.farZ)
    assert (gpu.peel("opaque", 1, prev, 0.5, 0, scene=gs) == np.float32(1.0)).all()
    assert (gpu.peel("opaque", 1, prev, 0.5, 1, scene=gs) == far).all()
    gs.release()


def _np(t):
    return t.cpu().numpy()


def test_graph_dual_depth_from_depth_peeling(oracle, checker, gpu):
    """tests/graphs/svao_dual_peel.py executed twice: DepthPeeling.depth2 is the checker's raster layer,
    LinearizeDepth0 linearises it, and SVAO (DualDepth, exact numerics) equals the oracle fed with it."""
    from rsd import graph as rg
    from rsd.frame import FrameConfig, make_vao, sd_params, svao_params
    O, c, torch = oracle, gpu.cases["opaque"], gpu.torch
    cfg = FrameConfig(visible_w=W - 16, visible_h=H - 16, guard_band=8, divisor=1, sd_guard_px=16, radius=2.0,
                      primary=gpu.abi.DEPTH_DUAL, numerics="exact")
    assert (cfg.fb_w, cfg.fb_h) == (W, H)
    vao, sd_w, sd_h = make_vao(cfg)

    def run(primary):
        g = rg.load_script(SCRIPT)["SVAODualPeel"]
        if primary != "DualDepth":
            g = rg.load_script(SCRIPT.read_text().replace("'DualDepth'", f"'{primary}'"))["SVAODualPeel"]
        g.set_scene(gpu.scenes["opaque"].h, c.cam)
        g.compile(W, H)
        g.execute()
        g.execute()
        torch.cuda.synchronize()
        names = ["DepthPeeling.depth2", "LinearizeDepth0.linearDepth", "SVAO.ao", "SVAO.stencil",
                 "SVAO.internalRayMin", "SVAO.internalRayMax"] if primary == "DualDepth" else ["SVAO.ao"]
        out = {n: _np(g.output_tensor(n)) for n in names}
        g.close()
        return out

    got = run("DualDepth")
    d, nw = O.gbuffer_raster(c.osc, c.ocam, W, H, 1)
    z = O.linearize_depth(d, c.ocam.nearZ, c.ocam.farZ)
    n = O.compress_normals(nw, c.ocam)
    d2 = DP.peel(O, checker, c, 1, z, 0.5, 0)
    np.testing.assert_array_equal(DP.bits(got["DepthPeeling.depth2"]).reshape(H, W), DP.bits(d2))
    z2 = O.linearize_depth(d2, c.ocam.nearZ, c.ocam.farZ)
    np.testing.assert_array_equal(DP.bits(got["LinearizeDepth0.linearDepth"]).reshape(H, W), DP.bits(z2))
    ovao, svp, sdp = to_oracle(vao, O.VAOData), to_oracle(svao_params(cfg), O.SVAOParams), \
        to_oracle(sd_params(cfg, vao.sdGuard), O.SDParams)
    ao1, st, rmin, rmax = O.svao_pass1(c.ocam, ovao, svp, z, n, sd_w, sd_h, depth2=z2)
    sd, _ = O.sd_trace(c.osc, c.ocam, sdp, z, rmin, rmax, sd_w, sd_h)
    ao = O.svao_pass2(c.ocam, ovao, svp, z, n, st, sd, ao1, depth2=z2)
    np.testing.assert_array_equal(got["SVAO.stencil"].reshape(H, W), st)
    np.testing.assert_array_equal(got["SVAO.internalRayMin"].view(np.uint32).reshape(sd_h, sd_w), rmin)
    np.testing.assert_array_equal(got["SVAO.internalRayMax"].view(np.uint32).reshape(sd_h, sd_w), rmax)
    np.testing.assert_array_equal(got["SVAO.ao"].reshape(H, W), ao)
    assert (run("SingleDepth")["SVAO.ao"] != got["SVAO.ao"]).any()


def test_renderer_depth_peel(oracle, checker, gpu):
    """gbuffer(); depth_peel(0.5); frame() on a DualDepth renderer: depth2 is the checker's linear layer and
    the AO is the oracle's frame with it; a SingleDepth renderer has no depth2 to fill."""
    from helpers import small_frame_config
    from rsd.frame import Renderer
    O, c = oracle, gpu.cases["opaque"]
    cfg = small_frame_config(visible=(W - 16, H - 16), guard=8, divisor=1, radius=2.0)
    cfg.sd_guard_px, cfg.primary, cfg.numerics = 16, gpu.abi.DEPTH_DUAL, "exact"
    r = Renderer(c.scene, cfg, gpu_scene=gpu.scenes["opaque"], dev=gpu.dev)
    r.gbuffer()
    r.depth_peel(0.5)
    r.frame()
    g = r.numpy()
    d2 = r.depth2.cpu().numpy()
    cam, vao = to_oracle(r.cam, O.Camera), to_oracle(r.vao, O.VAOData)
    sdp, svp = to_oracle(r.sdp, O.SDParams), to_oracle(r.svp, O.SVAOParams)
    z, n = O.gbuffer(c.osc, cam, W, H, cfg.cull_mode)
    np.testing.assert_array_equal(DP.bits(g["depth"]), DP.bits(z))
    want2 = DP.peel(O, checker, c, cfg.cull_mode, z, 0.5, 1, ocam=cam)
    np.testing.assert_array_equal(DP.bits(d2), DP.bits(want2))
    ao1, st, rmin, rmax = O.svao_pass1(cam, vao, svp, z, n, r.sd_w, r.sd_h, depth2=want2)
    sd, _ = O.sd_trace(c.osc, cam, sdp, z, rmin, rmax, r.sd_w, r.sd_h)
    ao = O.svao_pass2(cam, vao, svp, z, n, st, sd, ao1, depth2=want2)
    np.testing.assert_array_equal(g["stencil"], st)
    np.testing.assert_array_equal(g["ao"], ao)
    # cull_mode overrides the config's
    r.depth_peel(0.5, cull_mode=gpu.abi.CULL_NONE)
    np.testing.assert_array_equal(DP.bits(r.depth2.cpu().numpy()), DP.bits(DP.peel(O, checker, c, 0, z, 0.5, 1, ocam=cam)))
    cfg1 = small_frame_config(visible=(W - 16, H - 16), guard=8, divisor=1, radius=2.0)
    cfg1.sd_guard_px = 16
    single = Renderer(c.scene, cfg1, gpu_scene=gpu.scenes["opaque"], dev=gpu.dev)
    with pytest.raises(ValueError, match="DEPTH_DUAL"):
        single.depth_peel(0.5)
