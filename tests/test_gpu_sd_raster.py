"""GPU: rsd_sd_raster against the brute-force CPU checker (tests/native/sd_raster_ref.c, pinned to the oracle
by tests/test_sd_raster.py).  Every comparison is bitwise; the outputs are pre-filled with a sentinel so that
an unwritten texel shows.  75 x 45 frames of ~3000-triangle scenes: partial 8 x 8 tiles on both axes, SD maps
of 75 x 45, 38 x 23 and 25 x 15 texels.  The cases vary around sd_raster_checker.BASE one parameter at a
time; the intervals and the stencil are those of a real rsd_svao_pass1 on the same frame."""
import ctypes as C

import numpy as np
import pytest

import sd_raster_checker as SR

pytestmark = pytest.mark.gpu

W, H = SR.W, SR.H
B = SR.BASE
SENTINEL = -7.0


@pytest.fixture(scope="session")
def checker(oracle, tmp_path_factory):
    return SR.build(oracle, tmp_path_factory.mktemp("sd_raster_ref"))


class Gpu:
    """The two small scenes on the GPU and, per (scene, divisor), the frame the SD pass reads: the non-linear
    G-buffer depth and pass 1's intervals (computed once, never modified)."""

    def __init__(self, oracle):
        import torch
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from rsd import abi
        from rsd.frame import Device, GpuScene
        self.torch, self.abi = torch, abi
        self.dev = Device(0)
        self.cases = {k: SR.Case(oracle, k) for k in SR.SCENES}
        self.scenes = {k: GpuScene(self.dev, c.scene) for k, c in self.cases.items()}
        self._frames = {}

    def frame(self, kind=B["kind"], divisor=B["divisor"]):
        key = (kind, divisor)
        if key not in self._frames:
            from rsd.frame import Renderer
            t, abi, c = self.torch, self.abi, self.cases[kind]
            r = Renderer(c.scene, SR.frame_config(divisor, B["radius"], B["N"], B["cull"]),
                         gpu_scene=self.scenes[kind], dev=self.dev)
            r.cam = c.cam
            r.gbuffer()
            r.clear_intervals()
            r.pass1()
            d = t.empty((H, W), dtype=t.float32, device="cuda")
            nw = t.empty((H, W, 4), dtype=t.float32, device="cuda")
            p = lambda x: C.c_void_p(x.data_ptr())
            abi.check(abi.lib().rsd_gbuffer_raster(self.scenes[kind].h, C.byref(c.cam), W, H, B["cull"], p(d), p(nw),
                                                   None), "rsd_gbuffer_raster")
            g = r.numpy()
            f = dict(depth=d.cpu().numpy(), rmin=g["ray_min"].copy(), rmax=g["ray_max"].copy(), sd_w=r.sd_w,
                     sd_h=r.sd_h)
            for a in (f["depth"], f["rmin"], f["rmax"]):
                a.setflags(write=False)
            self._frames[key] = f
        return self._frames[key]

    def raster(self, kind, prm, depth, sd_w, sd_h, rmin=None, rmax=None, stencil=None, scene=None, status=None):
        t, abi = self.torch, self.abi
        N = prm.sample_count
        dev = lambda a, dt: None if a is None else t.from_numpy(np.array(a, dt)).cuda()
        d, lo, hi, st = dev(depth, np.float32), dev(rmin, np.int32), dev(rmax, np.int32), dev(stencil, np.uint8)
        shape = ((N + 3) // 4, sd_h, sd_w, min(N, 4)) if N in (1, 2, 4, 8, 16) else (1, sd_h, sd_w, 4)
        out = t.full(shape, SENTINEL, dtype=t.float32, device="cuda")
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        gp = abi.SDRasterParams.from_buffer_copy(prm)
        h = scene.h if scene is not None else self.scenes[kind].h
        s = abi.lib().rsd_sd_raster(h, C.byref(self.cases[kind].cam), C.byref(gp), p(d), depth.shape[1],
                                    depth.shape[0], p(lo), p(hi), p(st), p(out), sd_w, sd_h, None)
        t.cuda.synchronize()
        if status is not None:
            assert s == status, (s, abi.last_error())
            return out.cpu().numpy()
        abi.check(s, "rsd_sd_raster")
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


def compare(oracle, checker, gpu, kind=B["kind"], divisor=B["divisor"], intervals=True, stencil=None, **over):
    """One case: BASE with `over` applied to the pass's parameters.  Returns the checker's counters."""
    f = gpu.frame(kind, divisor)
    kw = dict(N=B["N"], alpha=B["alpha"], cull=B["cull"], use_stencil=True)
    kw.update(over)
    prm = SR.params(**kw)
    rmin, rmax = (f["rmin"].view(np.uint32), f["rmax"].view(np.uint32)) if intervals else (None, None)
    want, cnt = SR.raster(oracle, checker, gpu.cases[kind], prm, f["depth"], f["sd_w"], f["sd_h"], rmin, rmax, stencil)
    got = gpu.raster(kind, prm, f["depth"], f["sd_w"], f["sd_h"], rmin, rmax, stencil)
    assert got.shape == want.shape
    assert not (got == SENTINEL).any(), "unwritten texels"
    np.testing.assert_array_equal(SR.bits(got), SR.bits(want))
    return cnt, want


def test_base_case(oracle, checker, gpu):
    cnt, want = compare(oracle, checker, gpu)
    print("checker counters of the base case:", cnt)
    # no rule, and neither the stencil nor the stratified masks, is idle on this frame
    for k in SR.COUNTERS[1:]:
        assert cnt[k] >= SR.BASE_MINIMUM, (k, cnt)
    assert (want == 1.0).any() and (want < 1.0).any()


@pytest.mark.parametrize("N", [1, 2, 8, 16])
def test_sample_counts(oracle, checker, gpu, N):
    cnt, want = compare(oracle, checker, gpu, N=N)
    assert (want < 1.0).any() and (want == 1.0).any()


@pytest.mark.parametrize("divisor", [2, 3])
def test_divisors(oracle, checker, gpu, divisor):
    """2: the bilinear first layer; 3: point sampling on every third pixel; SD sizes 38 x 23 and 25 x 15."""
    f = gpu.frame(B["kind"], divisor)
    assert (f["sd_w"], f["sd_h"]) == (-(-W // divisor), -(-H // divisor))
    cnt, want = compare(oracle, checker, gpu, divisor=divisor)
    assert cnt["first_layer"] > 0 and (want < 1.0).any()


@pytest.mark.parametrize("cull", [1, 2])
def test_cull_modes(oracle, checker, gpu, cull):
    base_fragments = compare(oracle, checker, gpu)[0]["fragments"]
    cnt, _ = compare(oracle, checker, gpu, cull=cull)
    assert 0 < cnt["fragments"] < base_fragments


def test_non_linear_values(oracle, checker, gpu):
    _, want = compare(oracle, checker, gpu, linearize=False)
    _, lin = compare(oracle, checker, gpu)
    assert ((want < 1.0) == (lin < 1.0)).all() and (want[want < 1.0] != lin[want < 1.0]).any()


@pytest.mark.parametrize("alpha", [None, 1.0])
def test_alpha_values(oracle, checker, gpu, alpha):
    """1.5 / N (SVAO's): one or two samples per fragment; 1.0: the full mask."""
    cnt, _ = compare(oracle, checker, gpu, alpha=alpha)
    assert cnt["r_zero"] == 0


def test_without_intervals(oracle, checker, gpu):
    """RayInterval off with the maps given (rayMax is still the stencil), and no maps at all."""
    cnt, _ = compare(oracle, checker, gpu, ray_interval=False)
    assert cnt["ray_min"] == cnt["ray_max"] == 0 and cnt["stencilled"] >= SR.BASE_MINIMUM
    cnt, _ = compare(oracle, checker, gpu, intervals=False)
    assert cnt["ray_min"] == cnt["ray_max"] == cnt["stencilled"] == 0


def test_stencil_sources(oracle, checker, gpu):
    f = gpu.frame()
    cnt, _ = compare(oracle, checker, gpu, use_stencil=False)  # a depth format without stencil
    assert cnt["stencilled"] == 0
    mask = (np.random.default_rng(3).integers(0, 3, size=(f["sd_h"], f["sd_w"])) * 100).astype(np.uint8)
    cnt, want = compare(oracle, checker, gpu, stencil=mask)  # the explicit R8 mask wins over rayMax
    assert cnt["stencilled"] == int((mask == 0).sum()) >= SR.BASE_MINIMUM
    assert (want[:, mask == 0] == 1.0).all()
    cnt, _ = compare(oracle, checker, gpu, stencil=mask, use_stencil=False)
    assert cnt["stencilled"] == 0


def test_alpha_test_off_and_opaque_scene(oracle, checker, gpu):
    on, m_on = compare(oracle, checker, gpu)
    off, m_off = compare(oracle, checker, gpu, alpha_test=False)
    assert on["alpha"] >= SR.BASE_MINIMUM and off["alpha"] == 0 and (SR.bits(m_on) != SR.bits(m_off)).any()
    cnt, want = compare(oracle, checker, gpu, kind="opaque", intervals=False, alpha=None)
    assert cnt["alpha"] == 0 and (want < 1.0).sum() >= 100


def test_scene_without_triangles_is_all_cleared(gpu):
    from rsd.frame import GpuScene
    from rsd.scenes import Scene
    f = gpu.frame()
    empty = Scene("empty", np.zeros((1, 3), np.float32), np.zeros((0, 3), np.uint32), np.zeros(0, np.uint32),
                  gpu.cases["opaque"].scene.camera)
    gs = GpuScene(gpu.dev, empty)
    for N in (1, 8):
        got = gpu.raster("opaque", SR.params(N=N), f["depth"], 38, 23, scene=gs)
        assert (got == np.float32(1.0)).all()
    gs.release()


def test_refusals(gpu):
    abi, f = gpu.abi, gpu.frame()
    for prm, status in ((SR.params(implementation=abi.SD_RESERVOIR_SAMPLING), abi.ERR_UNSUPPORTED),
                        (SR.params(implementation=abi.SD_KBUFFER), abi.ERR_UNSUPPORTED),
                        (SR.params(N=3), abi.ERR_INVALID_ARG), (SR.params(cull=3), abi.ERR_INVALID_ARG)):
        got = gpu.raster(B["kind"], prm, f["depth"], f["sd_w"], f["sd_h"], status=status)
        assert (got == SENTINEL).all()  # nothing was launched
