"""GPU: every ray walk of librsd on the adversarial-geometry scenes (tests/scenes_adversarial.py), bit for bit
against the oracle, whose hit collection and G-buffer tests/test_adversarial_walk.py pins to brute force on
these very scenes, and against the brute-force checkers themselves (tests/native/hits_ref.c,
tests/native/depth_peel_ref.c).  65 x 49 frames, jitter off: the centre column and row are axis-parallel rays."""
import ctypes as C

import numpy as np
import pytest

import depth_peel_checker as DP
import hits_checker as HC
import scenes_adversarial as SA
from helpers import to_oracle

pytestmark = pytest.mark.gpu

W, H = HC.W, HC.H
D, CM, KB = 0, 1, 3  # rsd_sd_implementation: Default, CoverageMask, KBuffer

# (walk, N, MAX_COUNT, implementation): the sorted lists hold K = 4 / 8 / 16 keys for MAX_COUNT <= 4 / 8 / more
# (CoverageMask: 8, streamed in chunks), so MAX_COUNT 1 and 8 sit below and at K = 8, 16 at K = 16, 32 above it.
# "hybrid" is the default choice of a small map; "hybrid16" its K = 16 rows holding two keys per lane.
CANONICAL = [
    ("fused", 4, 1, D), ("fused", 8, 8, D), ("fused", 16, 16, D), ("fused", 4, 32, D), ("fused", 8, 8, KB),
    ("fused", 16, 32, KB), ("fused", 4, 8, CM), ("fused", 16, 32, CM),
    ("split", 1, 1, D), ("split", 4, 8, D), ("split", 8, 8, KB), ("split", 16, 16, D),
    ("quad", 1, 1, D), ("quad", 4, 8, D), ("quad", 16, 16, KB), ("quad", 8, 32, D), ("quad", 4, 8, CM),
    ("quad", 16, 16, D), ("quad", 8, 16, CM),
    ("hybrid", 4, 1, D), ("hybrid", 4, 8, D), ("hybrid", 8, 8, D),
    ("hybrid16", 16, 16, D), ("hybrid16", 8, 16, D),
    ("raster", 4, 8, D), ("raster", 16, 16, D), ("raster", 1, 1, KB),
]
ENTRY_WALKS = ("fused", "split", "quad")  # the walks the entry grid serves: run with it and from the root
ORDERED = [(1, 4, 8, D), (1, 16, 16, KB), (1, 4, 32, D), (1, 4, 8, CM), (1, 1, 1, D),
           (2, 4, 8, D), (2, 16, 16, KB), (2, 4, 32, D), (2, 4, 8, CM), (2, 1, 1, D)]
ENV = {"fused": dict(RSD_TRACE_WALK="fused", RSD_TRACE_HYBRID="off"),
       "split": dict(RSD_TRACE_WALK="split", RSD_TRACE_HYBRID="off"),
       "quad": dict(RSD_TRACE_WALK="quad", RSD_TRACE_HYBRID="off"),
       "hybrid": dict(), "hybrid16": dict(RSD_TRACE_HYBRID16="on"), "raster": dict(RSD_TRACE_WALK="raster")}
KNOBS = ("RSD_TRACE_WALK", "RSD_TRACE_HYBRID", "RSD_TRACE_HYBRID16", "RSD_TRACE_ENTRY", "RSD_TRACE_SPEC")


@pytest.fixture(scope="session")
def hits_lib(oracle, tmp_path_factory):
    return HC.build(oracle, tmp_path_factory.mktemp("hits_ref"))


@pytest.fixture(scope="session")
def peel_lib(oracle, tmp_path_factory):
    return DP.build(oracle, tmp_path_factory.mktemp("depth_peel_ref"))


class Gpu:
    """The scenes on the GPU (uploaded on first use) and one renderer per (scene, N, Use16Bit)."""

    def __init__(self, oracle):
        import torch
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from rsd import abi
        from rsd.frame import Device
        self.torch, self.abi, self.oracle = torch, abi, oracle
        self.dev = Device(0)
        self.cases, self.scenes, self.renderers = {}, {}, {}

    def case(self, name):
        if name not in self.cases:
            from rsd.frame import GpuScene
            self.cases[name] = HC.Case(self.oracle, name)
            self.scenes[name] = GpuScene(self.dev, self.cases[name].scene)
        return self.cases[name]

    def renderer(self, name, N, use16=False):
        key = (name, N, use16)
        if key not in self.renderers:
            from rsd.frame import Renderer
            c = self.case(name)
            r = Renderer(c.scene, SA.frame_config(N=N, use_16bit=use16), dev=self.dev, gpu_scene=self.scenes[name])
            r.depth.zero_()
            self.renderers[key] = r
        return self.renderers[key]

    def trace(self, monkeypatch, name, walk, N, max_count, impl, entry="on", hit_order=0, cull=1, normalize=0,
              rmin=None, rmax=None, use16=False, expect_walk=True):
        """One SD trace over a zero depth input; returns (the map, the oracle's parameter struct)."""
        t, abi = self.torch, self.abi
        r = self.renderer(name, N, use16)
        sdp = r.sdp
        sdp.max_count, sdp.implementation, sdp.hit_order, sdp.cull_mode, sdp.normalize = \
            max_count, impl, hit_order, cull, normalize
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in ENV[walk].items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("RSD_TRACE_ENTRY", entry)
        for dst, src in ((r.ray_min, rmin), (r.ray_max, rmax)):
            if src is None:
                dst.zero_()
            else:
                dst.copy_(t.from_numpy(np.ascontiguousarray(src, np.uint32).view(np.int32)))
        if expect_walk and hit_order == 0:
            split_ok = impl != CM and max_count <= (4 if max_count <= 4 else 8 if max_count <= 8 else 16)
            want = {"fused": abi.WALK_FUSED, "split": abi.WALK_SPLIT if split_ok else abi.WALK_FUSED,
                    "quad": abi.WALK_QUAD, "hybrid": abi.WALK_HYBRID, "hybrid16": abi.WALK_HYBRID,
                    "raster": abi.WALK_RASTER}[walk]
            got = int(r.sd_trace(counters=True).walk)
            assert got == want, (name, walk, N, max_count, impl, abi.WALK_NAMES[got])
        r.sd.fill_(-7.0)
        r.sd_trace()
        t.cuda.synchronize()
        return r.sd.cpu().numpy(), to_oracle(sdp, self.oracle.SDParams)

    def close(self):
        for s in self.scenes.values():
            s.release()
        self.dev.close()


@pytest.fixture(scope="module")
def gpu(oracle):
    g = Gpu(oracle)
    yield g
    g.close()


def differing(got, want):
    """The texels (y, x) of an SD map [layer][y][x][ch] whose bits differ, or None."""
    bad = (HC.bits(got) != HC.bits(want)).any(axis=(0, 3))
    return None if not bad.any() else f"{int(bad.sum())} texels, first (y, x) {np.argwhere(bad)[:4].tolist()}"


@pytest.mark.parametrize("name", SA.NAMES)
def test_canonical_walks_match_the_oracle(oracle, gpu, monkeypatch, name):
    """Every canonical walk x MAX_COUNT below, at and above its K x every implementation, with the entry grid and
    from the root: the oracle's map, bit for bit."""
    c = gpu.case(name)
    wants, failures = {}, []
    for walk, N, mc, impl in CANONICAL:
        for entry in (("on", "off") if walk in ENTRY_WALKS else ("on",)):
            got, sdp = gpu.trace(monkeypatch, name, walk, N, mc, impl, entry)
            if (N, mc, impl) not in wants:
                wants[N, mc, impl] = oracle.sd_trace(c.osc, c.ocam, sdp, c.depth, None, None, W, H)[0]
            bad = differing(got, wants[N, mc, impl])
            if bad:
                failures.append((walk, N, mc, impl, entry, bad))
    assert not failures, failures


@pytest.mark.parametrize("name", SA.NAMES)
def test_kbuffer_is_the_brute_force_list(oracle, hits_lib, gpu, monkeypatch, name):
    """KBuffer with MAX_COUNT above the list: the first 16 (8, 4) brute-force t * cosT per texel, with
    normalisation off, for Back and no culling."""
    c = gpu.case(name)
    for cull in (1, 0):
        cnt, _, _, zt = c.hits(oracle, hits_lib, cull)
        for walk, N in (("fused", 16), ("quad", 16), ("fused", 8), ("quad", 4)):
            got, _ = gpu.trace(monkeypatch, name, walk, N, 32, KB, cull=cull)
            # MAX_COUNT 32 ends a ray at its 32nd hit: the first N <= 16 slots are decided before that
            assert differing(got, HC.first_depths(cnt, zt, N)) is None, (walk, N, cull)


@pytest.mark.parametrize("name", SA.NAMES)
def test_traversal_and_wavefront_orders_match_the_oracle(oracle, gpu, monkeypatch, name):
    """The two any-hit orders librsd defines over its own tree (the oracle walks the exported BVH)."""
    c = gpu.case(name)
    bvh, off = gpu.scenes[name].export_bvh()
    soft = min(208 - 3 * int(gpu.scenes[name].info.wide_depth), 160)
    failures = []
    for order, N, mc, impl in ORDERED:
        got, sdp = gpu.trace(monkeypatch, name, "hybrid", N, mc, impl, hit_order=order)
        if order == 1:
            want = oracle.sd_trace_ordered(c.osc, bvh, off, c.ocam, sdp, c.depth, None, None, W, H)[0]
        else:
            want = oracle.sd_trace_wavefront(c.osc, bvh, off, soft, c.ocam, sdp, c.depth, None, None, W, H)[0]
        bad = differing(got, want)
        if bad:
            failures.append((order, N, mc, impl, bad))
    assert not failures, failures


@pytest.mark.parametrize("name", SA.NAMES)
def test_use16bit_and_normalised_maps(oracle, gpu, monkeypatch, name):
    """Use16Bit (N <= 4): the oracle's map rounded to binary16; and the normalised map of the default walk."""
    c = gpu.case(name)
    for N, mc in ((1, 1), (4, 8), (2, 32)):
        got, sdp = gpu.trace(monkeypatch, name, "hybrid", N, mc, D, use16=True, normalize=1, expect_walk=False)
        want = oracle.sd_trace(c.osc, c.ocam, sdp, c.depth, None, None, W, H)[0]
        assert got.dtype == np.float16
        np.testing.assert_array_equal(got.view(np.uint16), want.astype(np.float16).view(np.uint16))
        got32, _ = gpu.trace(monkeypatch, name, "hybrid", N, mc, D, normalize=1, expect_walk=False)
        assert differing(got32, want) is None, (N, mc)


def _next(a, up):
    a = np.ascontiguousarray(a, np.float32)
    return np.nextafter(a, np.float32(np.inf if up else -np.inf), dtype=np.float32)


@pytest.mark.parametrize("name", ["layers", "axis_walls", "far_a_layers", "far_b_layers", "far_a_axis_walls",
                                  "far_b_axis_walls"])
def test_exact_interval_ends(oracle, hits_lib, gpu, monkeypatch, name):
    """rayMin / rayMax written from the brute-force list itself (the depth input is zero, so TMin is the interval's):
    an end on the bits of the k-th hit's t keeps that hit and every hit tied with it, an end one float past it
    drops them.  The brute-force list of the clipped rays must confirm that before the GPU is compared."""
    c = gpu.case(name)
    cnt, t, _, _ = c.hits(oracle, hits_lib, 1)
    k = np.minimum((cnt.astype(np.int64) - 1) // 2, HC.CAP - 1)  # the middle hit of each texel's list
    tk = np.take_along_axis(t, np.maximum(k, 0)[..., None], 2)[..., 0]
    has = cnt > 0
    tk = np.where(has, tk, np.float32(1.0)).astype(np.float32)
    at = ((t == tk[..., None]) & (np.arange(HC.CAP) < cnt[..., None])).sum(-1)  # hits tied with it (itself included)
    word = lambda a: np.where(has, HC.bits(a), 0).astype(np.uint32)
    ends = {"both on the hit": (word(tk), word(tk)),
            "max just below": (None, word(_next(tk, False))),
            "max on the hit": (None, word(tk)),
            "min on the hit": (word(tk), None),
            "min just above": (word(_next(tk, True)), None)}
    failures = []
    for label, (rmin, rmax) in ends.items():
        n_ref = c.hits(oracle, hits_lib, 1, rmin, rmax)[0].astype(np.int64)
        lower = (t < tk[..., None]).sum(-1)  # hits strictly before the k-th
        if label == "both on the hit":
            np.testing.assert_array_equal(n_ref[has], at[has])
        elif label == "max just below":
            np.testing.assert_array_equal(n_ref[has], lower[has])
        elif label == "max on the hit":
            np.testing.assert_array_equal(n_ref[has], (lower + at)[has])
        elif label == "min on the hit":
            np.testing.assert_array_equal(n_ref[has], (cnt - lower)[has])
        else:
            np.testing.assert_array_equal(n_ref[has], (cnt - lower - at)[has])
        for walk, N, mc, impl in (("fused", 8, 8, D), ("quad", 16, 16, KB), ("hybrid", 4, 8, D), ("split", 4, 1, D),
                                  ("fused", 16, 32, KB), ("raster", 4, 8, D)):
            got, sdp = gpu.trace(monkeypatch, name, walk, N, mc, impl, rmin=rmin, rmax=rmax)
            want = oracle.sd_trace(c.osc, c.ocam, sdp, c.depth, rmin, rmax, W, H)[0]
            bad = differing(got, want)
            if bad:
                failures.append((label, walk, N, mc, impl, bad))
    assert has.mean() > 0.9
    assert not failures, failures


def _gbuffer(gpu, name, cull):
    t, abi, c = gpu.torch, gpu.abi, gpu.case(name)
    z = t.full((H, W), -7.0, dtype=t.float32, device="cuda")
    n = t.zeros((H, W), dtype=t.int16, device="cuda")
    abi.check(abi.lib().rsd_gbuffer(gpu.scenes[name].h, C.byref(c.cam), W, H, cull, C.c_void_p(z.data_ptr()),
                                    C.c_void_p(n.data_ptr()), None), "rsd_gbuffer")
    t.cuda.synchronize()
    return z.cpu().numpy(), n.cpu().numpy().view(np.uint16)


def _peel(gpu, name, cull, prev, sep):
    t, abi, c = gpu.torch, gpu.abi, gpu.case(name)
    pv = t.from_numpy(np.array(prev, np.float32)).cuda()
    out = t.full((H, W), -7.0, dtype=t.float32, device="cuda")
    abi.check(abi.lib().rsd_depth_peel(gpu.scenes[name].h, C.byref(c.cam), W, H, cull, C.c_void_p(pv.data_ptr()),
                                       float(sep), 1, C.c_void_p(out.data_ptr()), None), "rsd_depth_peel")
    t.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", SA.NAMES)
def test_gbuffer_and_depth_peel_match_brute_force(oracle, peel_lib, gpu, name):
    """rsd_gbuffer's depth and rsd_depth_peel (linear output) against tests/native/depth_peel_ref.c for every cull
    mode; the G-buffer's normals against the oracle's.  The peel runs with prev = 0 (nothing discarded: the walk of
    the stack model, so on `slivers` its spill arrays run), behind the first layer with separation 0 (strict at prev
    itself) and with the layer spacing 0.05, and behind the second layer with separation 0."""
    c = gpu.case(name)
    zero = np.zeros((H, W), np.float32)
    peel = lambda cull, prev, sep: DP.peel(oracle, peel_lib, c, cull, prev, sep, 1, width=W, height=H)
    for cull in (0, 1, 2):
        z, n = _gbuffer(gpu, name, cull)
        want_z, want_n = oracle.gbuffer(c.osc, c.ocam, W, H, cull)
        np.testing.assert_array_equal(DP.bits(z), DP.bits(peel(cull, zero, 0.0)))
        np.testing.assert_array_equal(DP.bits(z), DP.bits(want_z))
        np.testing.assert_array_equal(n, want_n)
        np.testing.assert_array_equal(DP.bits(_peel(gpu, name, cull, zero, 0.0)), DP.bits(z))
        second = peel(cull, z, 0.0)
        np.testing.assert_array_equal(DP.bits(_peel(gpu, name, cull, z, 0.0)), DP.bits(second))
        np.testing.assert_array_equal(DP.bits(_peel(gpu, name, cull, z, SA.LAYER_STEP)),
                                      DP.bits(peel(cull, z, SA.LAYER_STEP)))
        # prev + 0 exactly on the second layer: the third layer, never the second again
        third = peel(cull, second, 0.0)
        np.testing.assert_array_equal(DP.bits(_peel(gpu, name, cull, second, 0.0)), DP.bits(third))
        far = np.float32(c.ocam.farZ)
        assert ((third > second) | (second == far)).all()


@pytest.mark.parametrize("name", ["layers", "far_a_layers", "far_b_layers", "coincident", "slivers"])
def test_depth_peel_separation_lands_on_a_layer(oracle, hits_lib, peel_lib, gpu, name):
    """A non-zero separation whose float sum prev + separation is, bit for bit, the linear depth of a pixel's second
    hit: the strict predicate discards that hit.  The separation is the layer spacing 0.05; prev is chosen per pixel
    (one of the floats next to zlin - 0.05) so that the sum lands, and one float lower so that it falls short and the
    hit is kept.  Both facts are asserted on the brute-force reference before the GPU is compared with it."""
    c = gpu.case(name)
    sep = np.float32(SA.LAYER_STEP)
    cnt, _, _, zt = c.hits(oracle, hits_lib, 1)
    target = zt[..., 1]                                  # t * cosT of the second hit
    usable = (cnt >= 2) & (zt[..., 1] > zt[..., 0]) & np.isfinite(target) & (target > sep)
    target = np.where(usable, target, np.float32(1.0)).astype(np.float32)
    prev = (target - sep).astype(np.float32)
    for cand in (prev, np.nextafter(prev, np.float32(np.inf)), np.nextafter(prev, np.float32(-np.inf))):
        lands = (cand + sep).astype(np.float32) == target
        prev = np.where(lands & ~((prev + sep).astype(np.float32) == target), cand, prev).astype(np.float32)
    landed = usable & ((prev + sep).astype(np.float32) == target)
    print(name, ": prev + separation lands on the second hit at", int(landed.sum()), "of", int(usable.sum()), "pixels")
    assert landed.sum() >= 0.25 * W * H
    short = prev.copy()
    for _ in range(4):  # the nearest lower prev whose sum falls short of the hit
        low = (short + sep).astype(np.float32) >= target
        short = np.where(low, np.nextafter(short, np.float32(-np.inf)), short).astype(np.float32)
    assert ((short + sep).astype(np.float32) < target)[landed].all()
    want_on = DP.peel(oracle, peel_lib, c, 1, prev, float(sep), 1, width=W, height=H)
    want_short = DP.peel(oracle, peel_lib, c, 1, short, float(sep), 1, width=W, height=H)
    assert (want_on[landed] > target[landed]).all()      # dropped exactly at prev + separation
    np.testing.assert_array_equal(DP.bits(want_short)[landed], DP.bits(target)[landed])  # kept one float before it
    np.testing.assert_array_equal(DP.bits(_peel(gpu, name, 1, prev, sep)), DP.bits(want_on))
    np.testing.assert_array_equal(DP.bits(_peel(gpu, name, 1, short, sep)), DP.bits(want_short))


@pytest.mark.parametrize("kernel", ["vao", "hbao"])
@pytest.mark.parametrize("name,radius", [("layers", 1.0), ("axis_walls", 1.0), ("slivers", 1.0), ("slivers", 6.0)])
def test_raytraced_pass2_matches_the_oracle(oracle, gpu, name, radius, kernel):
    """SVAO pass 2 in the Raytraced secondary mode (its written-out copy of the per-lane walk, on secondary rays),
    exact numerics; on `slivers` also with AO rays long enough to cross many of the needles' boxes."""
    from rsd.frame import Renderer
    abi, c = gpu.abi, gpu.case(name)
    cfg = SA.frame_config(N=4, max_count=8, impl=D, radius=radius, ao_kernel=kernel)
    cfg.secondary = abi.DEPTH_RAYTRACED
    r = Renderer(c.scene, cfg, dev=gpu.dev, gpu_scene=gpu.scenes[name])
    r.gbuffer()
    r.frame()
    g = r.numpy()
    cam, vao, svp = to_oracle(r.cam, oracle.Camera), to_oracle(r.vao, oracle.VAOData), to_oracle(r.svp, oracle.SVAOParams)
    z, n = oracle.gbuffer(c.osc, cam, W, H, cfg.cull_mode)
    ao1, st, _, _ = oracle.svao_pass1(cam, vao, svp, z, n, r.sd_w, r.sd_h)
    np.testing.assert_array_equal(g["stencil"], st)
    assert (st != 0).sum() > 50, "no refined directions: the frame asks for no ray"
    ao = oracle.svao_pass2_raytraced(c.osc, cam, vao, svp, z, n, st, ao1, cull=cfg.cull_mode, ray_pipeline=1)
    np.testing.assert_array_equal(g["ao"], ao)
