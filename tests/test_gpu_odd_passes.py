"""GPU: the ray and raster passes outside the SVAO frame, and the SVAO leftovers, at frames off their grids, with
canaries around every output buffer.

tests/test_gpu_odd_geometry.py guards the SVAO frame's seven buffers; this module does the same for the rest of
librsd: rsd_gbuffer_raster, rsd_gbuffer_world, rsd_depth_peel and rsd_rtao (an 8 x 8 tile, one lane per pixel) at
helpers.PIXEL_SHAPES, rsd_rtao_pack (256 lanes) at counts around its block, rsd_sd_raster and its clear kernel on SD
maps derived from PIXEL_SHAPES with divisors 1, 2 and 3, rsd_hbao and rsd_temporal_depth_peel (a 64 x 4 block) at
helpers.BLOCK_SHAPES and the scissors that leave nothing or one texel, and on helpers.ODD_FRAMES
rsd_svao_pass2_raytraced with both grids and the interleaved band calls rsd_svao_pass1_band, rsd_sd_trace_band,
rsd_svao_pass2_band with bands that own nothing.

Every output buffer of every call is a helpers.Canary view pre-filled with the sentinel, checked after the call; the
inputs are plain tensors compared with their host copies afterwards.  Exact numerics; every comparison is bit for bit
against the CPU checkers (tests/native/*.c) or the oracle unless the test says otherwise.  tests/test_odd_passes.py
asserts on the references alone that every shape can show a fault (hits and misses, a second layer, darkened texels,
reprojected texels, a ray-pipeline grid that reaches the guard band, empty bands) and that the expected images are
sensitive to the mutant each test names."""
import ctypes as C
import types

import numpy as np
import pytest

import depth_peel_checker as DP
import hbao_checker as HB
import rtao_checker as RT
import sd_raster_checker as SR
import temporal_peel_checker as TP
import test_gpu_odd_geometry as OG
import test_odd_passes as CPU
from helpers import (HBAO_EMPTY_SCISSOR, HBAO_ONE_TEXEL_SCISSOR, HBAO_SHAPES, ODD_FRAMES, ODD_PASS_FAR,
                     ODD_PASS_RTAO_MAX_T, ODD_PASS_SD_SAMPLES, PACK_COUNTS, PACK_SPECIALS, PIXEL_SHAPES, SENTINEL,
                     TEMPORAL_PEEL_SHAPES, assert_canaries_intact, band_counts, band_rows, canary, hbao_odd_input,
                     odd_frame, odd_pass_case, pack_expected, pack_inputs, shape_id, visible_region)

pytestmark = pytest.mark.gpu

ctx = OG.ctx  # test_gpu_odd_geometry's module fixture: one device, arcade_tiny uploaded, its oracle twin
KINDS = CPU.KINDS
SHAPES = [f.name for f in ODD_FRAMES]
bits = DP.bits


@pytest.fixture(scope="session")
def dp(oracle, tmp_path_factory):
    return DP.build(oracle, tmp_path_factory.mktemp("depth_peel_ref"))


@pytest.fixture(scope="session")
def rt(oracle, tmp_path_factory):
    return RT.build(oracle, tmp_path_factory.mktemp("rtao_ref"))


@pytest.fixture(scope="session")
def sr(oracle, tmp_path_factory):
    return SR.build(oracle, tmp_path_factory.mktemp("sd_raster_ref"))


@pytest.fixture(scope="session")
def hb(tmp_path_factory):
    return HB.build(tmp_path_factory.mktemp("hbao_ref"))


@pytest.fixture(scope="session")
def tp(tmp_path_factory):
    return TP.build(tmp_path_factory.mktemp("temporal_peel_ref"))


@pytest.fixture(scope="module")
def gpu(ctx, oracle):
    """The scenes of the passes outside the SVAO frame on ctx's device: the ~3000-triangle arcade_tiny and the alpha
    scene of the checkers, and a scene without triangles."""
    from rsd import abi
    from rsd.frame import GpuScene
    from rsd.scenes import Scene
    first = {k: DP.Case(oracle, k) for k in KINDS}
    empty = Scene("empty", np.zeros((1, 3), np.float32), np.zeros((0, 3), np.uint32), np.zeros(0, np.uint32),
                  first["opaque"].scene.camera)
    g = types.SimpleNamespace(torch=ctx.torch, abi=abi, L=abi.lib(), O=oracle, dev=ctx.dev, cache={},
                              scenes={k: GpuScene(ctx.dev, c.scene) for k, c in first.items()})
    g.scenes["empty"] = GpuScene(ctx.dev, empty)
    yield g
    ctx.torch.cuda.synchronize()
    for s in g.scenes.values():
        s.release()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Inputs:
    """Plain device tensors of host arrays, checked for equality with their host copies after the call."""

    def __init__(self, torch, **arrays):
        self.torch = torch
        self.host = {k: np.ascontiguousarray(a) for k, a in arrays.items()}
        signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}
        self.dev = {k: torch.from_numpy(a.view(signed.get(a.dtype, a.dtype)).copy()).cuda()
                    for k, a in self.host.items()}

    def __getitem__(self, k):
        return _p(self.dev[k])

    def unchanged(self, what):
        for k, a in self.host.items():
            got = self.dev[k].cpu().numpy().view(a.dtype)
            assert np.array_equal(got.view(np.uint8), a.view(np.uint8)), f"{what}: the input {k} changed"


def _same(got, want, what):
    OG._same(np.ascontiguousarray(got), np.ascontiguousarray(want), what)


def _sentinel_like(a):
    return np.full(a.shape + (a.dtype.itemsize,), SENTINEL, np.uint8).view(a.dtype).reshape(a.shape)


# ---------------------------------------------------------------------------------- 1. the raster G-buffers

@pytest.mark.parametrize("cull", [0, 1], ids=["none", "back"])
@pytest.mark.parametrize("size", PIXEL_SHAPES, ids=shape_id)
@pytest.mark.parametrize("kind", KINDS)
def test_gbuffer_raster_and_world(oracle, dp, rt, gpu, kind, size, cull):
    """rsd_gbuffer_raster and rsd_gbuffer_world: depth and normal are oracle.gbuffer_raster's bits from both calls,
    posW is the RTAO checker's, (0, 0, 0, 0) on a miss.
    Mutant: a row stride of roundup8(W) (tests/test_odd_passes.py test_mutants_of_the_tile_kernels_show: it changes
    all three images at 7 x 3, 9 x 9 and 65 x 17); a bounds test of `<=` stores past a row's end, into the next
    row's first pixel or, from the last row, into the canary."""
    W, H = size
    f = CPU.tile_frame(oracle, dp, kind, size, cull)
    c, t, scene = f["case"], gpu.torch, gpu.scenes[kind]
    assert c.cam.farZ == ODD_PASS_FAR
    out = {"raster depth": canary(t, (H, W), t.float32), "raster normal": canary(t, (H, W, 4), t.float32),
           "depth": canary(t, (H, W), t.float32), "normal": canary(t, (H, W, 4), t.float32),
           "posW": canary(t, (H, W, 4), t.float32)}
    v = {k: _p(o.view) for k, o in out.items()}
    gpu.abi.check(gpu.L.rsd_gbuffer_raster(scene.h, C.byref(c.cam), W, H, cull, v["raster depth"], v["raster normal"],
                                           None), "rsd_gbuffer_raster")
    assert_canaries_intact(t, out, f"rsd_gbuffer_raster {size}")
    gpu.abi.check(gpu.L.rsd_gbuffer_world(scene.h, C.byref(c.cam), W, H, cull, v["depth"], v["normal"], v["posW"],
                                          None), "rsd_gbuffer_world")
    assert_canaries_intact(t, out, f"rsd_gbuffer_world {size}")
    got = {k: o.numpy() for k, o in out.items()}
    for k in ("raster depth", "depth"):
        _same(got[k], f["depth"], f"{kind} {size} cull {cull}: {k}")
    for k in ("raster normal", "normal"):
        _same(got[k], f["normal_w"], f"{kind} {size} cull {cull}: {k}")
    want = RT.posw(oracle, rt, c, cull, width=W, height=H)
    _same(got["posW"], want, f"{kind} {size} cull {cull}: posW")
    hit = got["depth"] < 1.0
    assert ((got["posW"][..., 3] == 1.0) == hit).all() and (got["posW"][~hit] == 0).all() and hit.any()


# ---------------------------------------------------------------------------------- 2. the depth peel

@pytest.mark.parametrize("cull", [0, 1, 2], ids=["none", "back", "front"])
@pytest.mark.parametrize("linear_out", [0, 1], ids=["raster_out", "linear_out"])
@pytest.mark.parametrize("size", PIXEL_SHAPES, ids=shape_id)
def test_depth_peel(oracle, dp, gpu, size, linear_out, cull):
    """rsd_depth_peel behind the oracle's linear first layer at separation 0.5, on the opaque and the alpha scene:
    the depth-peel checker's bits.  On the scene without triangles its 256-lane clear kernel fills W * H = 1, 21,
    64, 81 and 1105 elements with 1 or farZ.
    Mutant: a row stride of roundup8(W) (test_mutants_of_the_tile_kernels_show); a clear grid that is not rounded
    up leaves the last W * H % 256 elements at the sentinel."""
    W, H = size
    t = gpu.torch
    for kind in KINDS:
        f = CPU.tile_frame(oracle, dp, kind, size, 1)
        c = f["case"]
        inp = Inputs(t, prev=f["z"])
        out = {"depth2": canary(t, (H, W), t.float32)}
        gpu.abi.check(gpu.L.rsd_depth_peel(gpu.scenes[kind].h, C.byref(c.cam), W, H, cull, inp["prev"], 0.5, linear_out,
                                           _p(out["depth2"].view), None), "rsd_depth_peel")
        assert_canaries_intact(t, out, f"rsd_depth_peel {kind} {size}")
        inp.unchanged(f"rsd_depth_peel {kind} {size}")
        want = f["second"][cull] if linear_out else DP.peel(oracle, dp, c, cull, f["z"], 0.5, 0, width=W, height=H)
        _same(out["depth2"].numpy(), want, f"{kind} {size} cull {cull} linear_out {linear_out}")
    out["depth2"].fill()
    gpu.abi.check(gpu.L.rsd_depth_peel(gpu.scenes["empty"].h, C.byref(c.cam), W, H, cull, inp["prev"], 0.5, linear_out,
                                       _p(out["depth2"].view), None), "rsd_depth_peel")
    assert_canaries_intact(t, out, f"rsd_depth_peel's clear {size}")
    inp.unchanged(f"rsd_depth_peel's clear {size}")
    cleared = np.float32(c.cam.farZ) if linear_out else np.float32(1.0)
    _same(out["depth2"].numpy(), np.full((H, W), cleared, np.float32), f"the clear at {size}")


# ---------------------------------------------------------------------------------- 3. RTAO

def _rtao_inputs(oracle, dp, rt, size):
    """The checker's world positions and the oracle's face normals of the opaque case (the pass's G-buffer)."""
    f = CPU.tile_frame(oracle, dp, "opaque", size, 1)
    return f["case"], RT.posw(oracle, rt, f["case"], 1, width=size[0], height=size[1]), f["normal_w"]


def _rtao(gpu, c, pw, nw, prm, frame, what):
    t = gpu.torch
    h, w = pw.shape[:2]
    inp = Inputs(t, posW=pw, normal=nw)
    out = {"ambient": canary(t, (h, w), t.float32), "ray distance": canary(t, (h, w), t.float32),
           "ray log": canary(t, (h, w, prm.spp, 4), t.float32)}
    gpu.abi.check(gpu.L.rsd_rtao(gpu.scenes["opaque"].h, C.byref(prm), w, h, inp["posW"], inp["normal"], frame,
                                 _p(out["ambient"].view), _p(out["ray distance"].view), _p(out["ray log"].view), None),
                  "rsd_rtao")
    assert_canaries_intact(t, out, what)
    inp.unchanged(what)
    return tuple(out[k].numpy() for k in ("ambient", "ray distance", "ray log"))


def _t_max(gpu, prm):
    v = C.c_float()
    gpu.abi.check(gpu.L.rsd_rtao_ray_t_max(C.byref(prm), C.byref(v)), "rsd_rtao_ray_t_max")
    return np.float32(v.value)


@pytest.mark.parametrize("frame", [0, 7])
@pytest.mark.parametrize("size", PIXEL_SHAPES, ids=shape_id)
def test_rtao_one_sample(oracle, dp, rt, gpu, size, frame):
    """rsd_rtao at spp = 1 without falloff: ambient, ray distance and the ray log (4 floats per pixel) are the
    checker's bits at frame indices 0 and 7.
    Mutant: a row stride of roundup8(W), or a pixel hashed with the padded width (the directions come from
    hash(x, y, frame)); test_mutants_of_the_tile_kernels_show has the stride on the G-buffer images these rays start
    from, and tests/test_odd_passes.py test_rtao_rays_hit_and_miss that hits and misses both occur."""
    c, pw, nw = _rtao_inputs(oracle, dp, rt, size)
    prm = gpu.abi.RTAOParams(max_t_hit=ODD_PASS_RTAO_MAX_T, apply_exponential_falloff=False)
    tmax = _t_max(gpu, prm)
    assert tmax == np.float32(ODD_PASS_RTAO_MAX_T)
    got = _rtao(gpu, c, pw, nw, prm, frame, f"rsd_rtao {size} frame {frame}")
    orig, d = RT.origins(rt, pw, nw, prm.normal_scale), RT.dirs(rt, pw, nw, frame)
    tr = RT.trace(oracle, rt, c.osc, c.has_alpha, orig, d, tmax)
    want = (RT.ambient_no_falloff(tr[..., 0], prm.minimum_ambient_illumination), RT.ray_distance(tr, tmax),
            np.concatenate([d[..., None, :3], tr[..., None]], -1))
    for g, w, name in zip(got, want, ("ambient", "ray distance", "ray log")):
        _same(g, w, f"{size} frame {frame}: {name}")


def test_rtao_four_samples_one_over_a_tile(oracle, dp, rt, gpu):
    """9 x 9 at spp = 4 with the falloff: the ray log has 16 floats per pixel, so its canary and its comparison catch
    a pixel stride of 4.  The logged directions are the float64 restatement of the generator within 1e-5 per
    component (the bound tests/test_gpu_rtao.py test_four_samples states), the logged t is the checker's trace of
    the logged directions bit for bit, the ray distance is (maxAORayTHit + the sum) / 4 bit for bit, and the ambient
    term is the float64 formula on the logged t within 1e-6 (test_falloff's bound there).
    Mutant: ray i of pixel o logged at entry o + i in place of spp o + i
    (tests/test_odd_passes.py test_mutant_of_the_rtao_ray_log_shows, on the checker's own log)."""
    size, frame = (9, 9), 3
    c, pw, nw = _rtao_inputs(oracle, dp, rt, size)
    prm = gpu.abi.RTAOParams(max_t_hit=ODD_PASS_RTAO_MAX_T, spp=4, apply_exponential_falloff=True)
    tmax = _t_max(gpu, prm)
    amb, dist, log = _rtao(gpu, c, pw, nw, prm, frame, "rsd_rtao 9 x 9 spp 4")
    valid = pw[..., 3] != 0
    assert log.shape == (9, 9, 4, 4) and valid.any() and not valid.all()
    err = np.abs(log[..., :3].astype(np.float64) - RT.dirs_float64(nw, frame, 4))[valid]
    print("spp 4 at 9 x 9: max direction error", err.max())
    assert err.max() <= 1e-5
    assert (log[~valid] == 0).all()
    orig = RT.origins(rt, pw, nw, prm.normal_scale)
    dirs4 = np.concatenate([log[..., :3], np.zeros_like(log[..., :1])], -1)
    tr = RT.trace(oracle, rt, c.osc, c.has_alpha, orig, dirs4, tmax)
    _same(log[..., 3], tr, "logged t")
    want = RT.ray_distance(tr, tmax)
    want[~valid] = tmax
    _same(dist, want, "ray distance")
    lam = np.float64(prm.exponential_falloff_decay_constant)
    t64 = log[..., 3].astype(np.float64)
    occ = np.exp(-lam * (t64 / np.float64(prm.max_t_hit)) ** 2)
    per_ray = np.where(t64 > 0, 1.0 - (1.0 - np.float64(np.float32(prm.minimum_ambient_illumination))) * occ, 1.0)
    aerr = np.abs(amb.astype(np.float64) - per_ray.mean(-1))
    print("spp 4 at 9 x 9: max ambient error", aerr.max())
    assert aerr.max() <= 1e-6
    assert (amb[~valid] == 1).all() and (dist[~valid] == tmax).all()


# ---------------------------------------------------------------------------------- 4. the pack kernel

@pytest.mark.parametrize("pairs", ["both", "ambient", "distance"])
@pytest.mark.parametrize("count", PACK_COUNTS)
def test_rtao_pack(gpu, count, pairs):
    """rsd_rtao_pack: floor(255 a + 0.5) and numpy's float16 rounding (tests/test_gpu_rtao.py test_graph), with both
    pairs of pointers, the ambient pair alone and the distance pair alone; the pair that is not passed keeps its
    sentinel bytes.  The distance input starts with NaN, +inf, 65520 and 70000 (above 65504: +inf), -0, 65504 and the
    float below 65520 (both 65504): the kernel's conversion is numpy's on all of them, bit for bit -- the quiet NaN
    0x7e00, 0x7c00, 0x8000 (printed below) -- so rsd.h's "round to nearest even" needs no further word.
    Mutant: a grid of count / 256 blocks (tests/test_odd_passes.py test_mutant_of_the_pack_kernel_shows)."""
    t = gpu.torch
    amb, dist = pack_inputs(count)
    a8, d16 = pack_expected(amb, dist)
    inp = Inputs(t, ambient=amb, distance=dist)
    out = {"ambient8": canary(t, (count,), t.uint8), "distance16": canary(t, (count,), t.int16)}
    use_a, use_d = pairs != "distance", pairs != "ambient"
    gpu.abi.check(gpu.L.rsd_rtao_pack(inp["ambient"] if use_a else None, inp["distance"] if use_d else None, count,
                                      _p(out["ambient8"].view) if use_a else None,
                                      _p(out["distance16"].view) if use_d else None, None), "rsd_rtao_pack")
    assert_canaries_intact(t, out, f"rsd_rtao_pack {count} {pairs}")
    inp.unchanged(f"rsd_rtao_pack {count} {pairs}")
    got8, got16 = out["ambient8"].numpy(), out["distance16"].numpy().view(np.uint16)
    n = min(count, len(PACK_SPECIALS))
    if use_d:
        print("count", count, "specials", PACK_SPECIALS[:n], "kernel", [hex(v) for v in got16[:n]], "numpy",
              [hex(v) for v in d16[:n]])
        assert np.array_equal(got16, d16), np.flatnonzero(got16 != d16)[:8]
    else:
        assert out["distance16"].untouched()
    if use_a:
        assert np.array_equal(got8, a8), np.flatnonzero(got8 != a8)[:8]
    else:
        assert out["ambient8"].untouched()


# ---------------------------------------------------------------------------------- 5. the raster SD map

def _sd_frames(oracle, sr, gpu):
    if "sd" not in gpu.cache:
        gpu.cache["sd"] = {(size, divisor): (case, fr) for size, divisor, case, fr in CPU.sd_raster_frames(oracle, sr)}
    return gpu.cache["sd"]


@pytest.mark.parametrize("N", ODD_PASS_SD_SAMPLES)
@pytest.mark.parametrize("size", PIXEL_SHAPES, ids=shape_id)
def test_sd_raster(oracle, sr, gpu, size, N):
    """rsd_sd_raster on sd_raster_checker's base case (alpha scene, no culling, Alpha 0.2, the stencil, pass 1's
    intervals from the oracle) at the frame `size` with divisors 1, 2 and 3 -- maps of 1 x 1 to 65 x 17 texels, below
    a tile, exactly a tile, one over -- and N = 1, 4 and 16: one and four layers ((N + 3) / 4, h, w, min(N, 4)) inside
    one canary.  The checker's bits; then the clear kernel on the scene without triangles.
    Mutant: a layer stride of roundup8(w) * roundup8(h) texels, which with four layers stores past the map (the
    canary) and moves layers 1 to 3 (the comparison); a row stride of roundup8(w) as for the other tile kernels
    (tests/test_odd_passes.py test_mutants_of_the_raster_sd_show, on the checker's maps at N = 16)."""
    t, B = gpu.torch, SR.BASE
    for divisor in (1, 2, 3):
        case, fr = _sd_frames(oracle, sr, gpu)[size, divisor]
        prm = SR.params(N=N, alpha=B["alpha"], cull=B["cull"], use_stencil=True)
        want, cnt = SR.raster(oracle, sr, case, prm, fr.depth, fr.sd_w, fr.sd_h, fr.rmin, fr.rmax)
        inp = Inputs(t, depth=fr.depth, rmin=fr.rmin, rmax=fr.rmax)
        out = {"sd": canary(t, want.shape, t.float32)}
        gp = gpu.abi.SDRasterParams.from_buffer_copy(prm)
        what = f"rsd_sd_raster {size} / {divisor} N {N}"
        for scene in ("alpha", "empty"):
            out["sd"].fill()
            gpu.abi.check(gpu.L.rsd_sd_raster(gpu.scenes[scene].h, C.byref(case.cam), C.byref(gp), inp["depth"],
                                              fr.depth.shape[1], fr.depth.shape[0], inp["rmin"], inp["rmax"], None,
                                              _p(out["sd"].view), fr.sd_w, fr.sd_h, None), "rsd_sd_raster")
            assert_canaries_intact(t, out, f"{what} ({scene} scene)")
            inp.unchanged(what)
            _same(out["sd"].numpy(), want if scene == "alpha" else np.ones_like(want), f"{what} ({scene} scene)")


# ---------------------------------------------------------------------------------- 6. the 64 x 4-block kernels

@pytest.mark.parametrize("exponent", HB.EXPONENTS)
@pytest.mark.parametrize("mode", [HB.SINGLE, HB.DUAL], ids=["SingleDepth", "DualDepth"])
@pytest.mark.parametrize("shape", HBAO_SHAPES + [HBAO_EMPTY_SCISSOR, HBAO_ONE_TEXEL_SCISSOR], ids=shape_id)
def test_hbao(hb, gpu, shape, mode, exponent):
    """rsd_hbao: the whole (16, qh, qw, 2) buffer is the checker's, scissored texels keep the sentinel, and with the
    empty scissor (40 x 24, guard band 16) every byte does; with the one-texel scissor (44 x 44, guard band 20) all
    but texel (5, 5) of each layer.  At 3 x 2 ten of the sixteen 1 x 1 layers hold no pixel of the image and are
    shaded like any other.
    Mutant: a scissor test of `<=`, or a row stride of roundup64(qw)
    (tests/test_odd_passes.py test_mutants_of_the_block_kernels_show)."""
    W, H, guard = shape
    t = gpu.torch
    s, radius = hbao_odd_input(HB, W, H)
    want, flags = HB.hbao(hb, s["layers"], s["layers2"], s["normal_w"], s["cam"], radius=radius, exponent=exponent,
                          depth_mode=mode, guard_band=guard, fill=SENTINEL)
    inp = Inputs(t, layers=s["layers"], layers2=s["layers2"], normal=s["normal_w"])
    out = {"ambient layers": canary(t, want.shape, t.uint8)}
    prm = gpu.abi.HBAOParams(radius=radius, power_exponent=exponent, depth_mode=mode, guard_band=guard)
    gpu.abi.check(gpu.L.rsd_hbao(inp["layers"], inp["layers2"] if mode == HB.DUAL else None, inp["normal"], W, H,
                                 C.byref(s["cam"]), C.byref(prm), _p(out["ambient layers"].view), None), "rsd_hbao")
    assert_canaries_intact(t, out, f"rsd_hbao {shape}")
    inp.unchanged(f"rsd_hbao {shape}")
    got = out["ambient layers"].numpy()
    diff = (got != want).any(-1)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5], got[diff][:5], want[diff][:5], flags[diff][:5])
    scissored = (flags & HB.SCISSORED) != 0
    assert scissored.sum() == HB.scissored_texels(W, H, guard)
    assert (got[scissored] == SENTINEL).all() and not (got[~scissored] == SENTINEL).all(-1).any()
    if shape == HBAO_EMPTY_SCISSOR:
        assert out["ambient layers"].untouched()
    if shape == HBAO_ONE_TEXEL_SCISSOR:
        assert (~scissored).sum() == 16


@pytest.mark.parametrize("pose", TP.POSES)
@pytest.mark.parametrize("size", TEMPORAL_PEEL_SHAPES, ids=shape_id)
def test_temporal_depth_peel(tp, gpu, size, pose):
    """rsd_temporal_depth_peel at the checker's separations and iteration counts: the checker's bits, every pixel of
    the sentinel-filled output written; and the first frame (no previous layer: a history of zeros, what
    rsd.temporal.TemporalDepthPeel passes) gives the first layer's bits.
    Mutant: a row stride of roundup64(W) (test_mutants_of_the_block_kernels_show)."""
    W, H = size
    t = gpu.torch
    s = TP.synthetic(tp, *size, pose)
    c2p, p2c = np.ascontiguousarray(s["c2p"], np.float32), np.ascontiguousarray(s["p2c"], np.float32)
    inp = Inputs(t, z=s["z"], prev=s["prev2"], none=np.zeros_like(s["z"]))
    out = {"depth2": canary(t, (H, W), t.float32)}

    def run(prev, sep, iterations):
        out["depth2"].fill()
        gpu.abi.check(gpu.L.rsd_temporal_depth_peel(inp["z"], inp[prev], W, H, C.byref(s["cam"]),
                                                    c2p.ctypes.data_as(C.c_void_p), p2c.ctypes.data_as(C.c_void_p),
                                                    sep, iterations, _p(out["depth2"].view), None),
                      "rsd_temporal_depth_peel")
        assert_canaries_intact(t, out, f"rsd_temporal_depth_peel {size} {pose} {sep} {iterations}")
        return out["depth2"].numpy()

    for sep in TP.SEPARATIONS:
        for iterations in TP.ITERATIONS:
            got = run("prev", sep, iterations)
            want, _ = TP.peel(tp, s["z"], s["prev2"], s["cam"], c2p, p2c, sep, iterations)
            assert (bits(got) != bits(_sentinel_like(got))).all(), "a pixel was not written"
            _same(got, want, f"{size} {pose} separation {sep} iterations {iterations}")
    _same(run("none", 0.5, 32), s["z"], f"{size} {pose}: the first frame")
    inp.unchanged(f"rsd_temporal_depth_peel {size} {pose}")


# ---------------------------------------------------------------------------------- 7. the SVAO leftovers

@pytest.mark.parametrize("cull", [0, 1], ids=["none", "back"])
@pytest.mark.parametrize("ray_pipeline", [0, 1], ids=["visible", "ray_pipeline"])
@pytest.mark.parametrize("name", SHAPES)
def test_pass2_raytraced(ctx, name, ray_pipeline, cull):
    """rsd_svao_pass2_raytraced (alpha test on) after its own G-buffer and pass 1 on a renderer configured with
    secondary = DEPTH_RAYTRACED: the whole AO buffer, guard band included, is oracle.svao_pass2_raytraced on the GPU's
    own stencil and pass-1 AO.  With ray_pipeline = 0 nothing outside the visible region changes; with
    ray_pipeline = 1 nothing left of or above the guard band.
    The ray-pipeline grid runs to the frame's edge, past the roundup32(visible) pixels that pass 1 dispatches
    (odd_div3: columns 165 and 166).  The reference's stencil holds its cleared 0 there (SVAO.cpp:307), and so does
    this test's: the stencil texels outside pass 1's dispatch are zeroed before the call, the AO keeps the sentinel.
    With the sentinel 0xA5 left in those stencil texels kernel and oracle differed on 70 pixels of column 165 at
    odd_div3.  The cause, read from the code: the sentinel sets direction bits that pass 1 rejects for such a pixel;
    for a rejected direction sample_init (csrc/svao_math.h) returns false before it fills the sample's ip, su, sv
    and isInScreen, rt_dir (csrc/svao_rt.hip) does not look at that result and traces with them uninitialised, while
    the oracle's o_sample_init fills them.  Pass 1 never sets such a bit, so the input is outside the contract,
    which include/rsd.h now states.
    Mutant: the ray-pipeline grid stops at the visible edge -- the other grid's image, which differs on every shape
    with a guard band (tests/test_odd_passes.py test_raytraced_pass2_changes_the_frame; `no_guards` has no guard band
    and cannot tell the grids apart)."""
    from rsd import abi
    r = OG._renderer(ctx, odd_frame(name), secondary=abi.DEPTH_RAYTRACED, ray_pipeline=bool(ray_pipeline),
                     cull_mode=cull)
    cfg, g0 = r.cfg, r.cfg.guard_band
    depth, normals = OG._gbuffer(ctx, r, cull)
    p1 = OG._pass1(ctx, r)
    reach = np.zeros(p1["stencil"].shape, bool)  # pass 1's dispatch: roundup32(visible) from the first visible pixel
    reach[g0:g0 + (cfg.visible_h + 31) // 32 * 32, g0:g0 + (cfg.visible_w + 31) // 32 * 32] = True
    p1["stencil"] = np.where(reach, p1["stencil"], 0).astype(p1["stencil"].dtype)
    OG._upload(ctx, r.stencil, p1["stencil"])
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    abi.check(abi.lib().rsd_svao_pass2_raytraced(r.gscene.h, C.byref(r.cam), C.byref(r.vao), C.byref(r.svp), p(r.depth),
                                                 p(r.normals), cfg.fb_w, cfg.fb_h, p(r.stencil), p(r.ao), cull,
                                                 ray_pipeline, 1, r.stream), "rsd_svao_pass2_raytraced")
    OG._intact(ctx, r, f"ray-traced pass 2 {name}")
    g = r.numpy()
    _same(g["depth"], depth, "the input depth")
    _same(g["normals"], normals, "the input normals")
    _same(g["stencil"], p1["stencil"], "the input stencil")
    cam, vao, _, svp = OG._structs(ctx, r)
    want = ctx.O.svao_pass2_raytraced(ctx.osc, cam, vao, svp, depth, normals, p1["stencil"], p1["ao"], cull=cull,
                                      ray_pipeline=ray_pipeline, alpha_test=1)
    _same(g["ao"], want, f"{name} ray_pipeline {ray_pipeline} cull {cull}: AO")
    assert not np.array_equal(g["ao"], p1["ao"]), "the rays changed nothing"
    changed = g["ao"] != p1["ao"]
    if ray_pipeline == 0:
        outside = np.ones(changed.shape, bool)
        outside[visible_region(cfg)] = False
        assert not changed[outside].any(), "the visible-pixel grid wrote outside the visible region"
    elif g0:
        assert not changed[:g0].any() and not changed[:, :g0].any(), "a store left of or above the guard band"


def _owned(spans, n):
    m = np.zeros(n, bool)
    for lo, hi in spans:
        m[lo:hi] = True
    return m


def _rows_kept(before, after, owned, what):
    assert np.array_equal(before[~owned], after[~owned]), f"{what}: rows of another band changed"


@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("which", [0, 1, 2], ids=["B2", "B3", "groups_plus_1"])
@pytest.mark.parametrize("name", SHAPES)
def test_bands(ctx, name, which, order):
    """rsd_svao_pass1_band, rsd_sd_trace_band and rsd_svao_pass2_band for every band b of B = 2, 3 and (32-row groups
    + 1), in ascending and in descending b: after all bands the five buffers are the whole-frame calls' bits
    (test_gpu_odd_geometry's _base), after each band the rows it does not own are unchanged, a band that owns nothing
    returns RSD_OK and changes no byte, band_index >= band_count and band_count = 0 are refused.
    Mutant: the 32-row groups counted from the frame's first row in place of the first visible row: with a guard
    band that is no multiple of 32 (every shape with one, tests/test_odd_passes.py test_band_rows) a band then
    stores rows of another band."""
    from rsd import abi
    L = abi.lib()
    f = odd_frame(name)
    b = OG._base(ctx, name)
    r = OG._renderer(ctx, f)
    cfg = r.cfg
    g0, vh, H = cfg.guard_band, cfg.visible_h, cfg.fb_h
    B = band_counts(f)[which]
    rows = band_rows(f, B)
    bands = list(range(B)) if order == "ascending" else list(range(B))[::-1]
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def trace_band(i, n):
        return L.rsd_sd_trace_band(r.gscene.h, C.byref(r.cam), C.byref(r.sdp), p(r.depth), cfg.fb_w, cfg.fb_h,
                                   p(r.ray_min), p(r.ray_max), p(r.sd), r.sd_w, r.sd_h, i, n, None, r.stream)

    OG._upload(ctx, r.depth, b.depth)
    OG._upload(ctx, r.normals, b.normals)
    for k in ("ao", "stencil", "ray_min", "ray_max", "sd"):
        r.canaries[k].fill()
    before = r.numpy()
    for i, n in ((B, B), (B + 1, B), (0, 0)):  # refused: no kernel runs, no byte changes
        for call in (r.pass1, r.pass2):
            with pytest.raises(abi.RsdError) as e:
                call(band=(i, n))
            assert e.value.status == abi.ERR_INVALID_ARG
        assert trace_band(i, n) == abi.ERR_INVALID_ARG
        OG._intact(ctx, r, f"refused band {i} of {n}")
        after = r.numpy()
        for k, a in before.items():
            _same(after[k], a, f"refused band {i} of {n}: {k}")
    r.clear_intervals()
    OG._intact(ctx, r, "interval clear")

    def step(call, i, what, keys, owned_rows):
        before = r.numpy()
        call(i)
        OG._intact(ctx, r, what)
        after = r.numpy()
        for k in ("depth", "normals", "ao", "stencil", "ray_min", "ray_max", "sd"):
            if k not in keys or not owned_rows.any():
                _same(after[k], before[k], f"{what}: {k} (not this call's to write)")
        return before, after

    # pass 1: a band stores the rows of its 32-row groups (the last group runs to roundup32 or the buffer's end)
    for i in bands:
        owned = _owned([(g0 + 32 * g, min(g0 + 32 * g + 32, H)) for g in rows[i][0]], H)
        before, after = step(lambda i: r.pass1(band=(i, B)), i, f"pass 1 band {i} of {B}",
                             ("ao", "stencil", "ray_min", "ray_max"), owned)
        for k in ("ao", "stencil"):
            _rows_kept(before[k], after[k], owned, f"pass 1 band {i} of {B}: {k}")
    OG._same_pass1(r.numpy(), b.g1, f"{name}: pass 1 in {B} bands")

    # the SD trace: a band stores its 8-row tile rows
    for i in bands:
        owned = _owned([(8 * t, min(8 * t + 8, r.sd_h)) for t in rows[i][1]], r.sd_h)
        before, after = step(lambda i: abi.check(trace_band(i, B), "rsd_sd_trace_band"), i,
                             f"SD trace band {i} of {B}", ("sd",), owned)
        _rows_kept(before["sd"].transpose(1, 0, 2, 3), after["sd"].transpose(1, 0, 2, 3), owned,
                   f"SD trace band {i} of {B}")
    _same(r.numpy()["sd"], b.gsd, f"{name}: SD trace in {B} bands")

    # pass 2: a band refines its visible rows only
    for i in bands:
        owned = _owned([(g0 + 32 * g, g0 + min(32 * g + 32, vh)) for g in rows[i][0]], H)
        before, after = step(lambda i: r.pass2(band=(i, B)), i, f"pass 2 band {i} of {B}", ("ao",), owned)
        _rows_kept(before["ao"], after["ao"], owned, f"pass 2 band {i} of {B}")
    _same(r.numpy()["ao"], b.gao, f"{name}: pass 2 in {B} bands")
    OG._same_pass1(dict(r.numpy(), ao=b.g1["ao"]), b.g1, f"{name}: pass 2 left stencil and intervals alone")
