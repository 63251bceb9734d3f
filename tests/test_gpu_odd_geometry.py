"""The SVAO frame at odd frame geometry, with canaries around every output buffer.

Every other small GPU frame of the suite has visible sizes that are multiples of 8, guard bands of 0 / 8 / 16 / 32,
divisors 1 / 2 / 4 and an SD guard the divisor divides.  helpers.ODD_FRAMES are the frames away from that: odd prime
sizes, odd guard bands, divisor 3, sdGuard = 7 / 3, no guard at all (the generic pass 1), a frame smaller than one
32 x 32 workgroup, a frame one pixel over a multiple of 32; tests/test_odd_geometry.py checks on the oracle alone that
each of them requests SD rays, stores into the guard band and has an SD map that is no multiple of the 8 x 8 tile.

Every output buffer of every call -- depth, normals, AO, stencil, rayMin, rayMax, the SD map -- is a view into a
larger allocation with at least 64 elements of sentinel before and after it, checked after every stage; a buffer whose
stage does not define every texel (pass 1 leaves the left and top guard band alone) is pre-filled with the sentinel,
and so is the oracle's.  Exact numerics; every comparison is bit for bit against the oracle over the WHOLE buffer,
guard band included.

The reference at these edges (what the oracle restates, rsd_oracle.c o_pass1_impl): "AO 1" is a compute dispatch of
roundup32(visible size) threads from the first visible pixel (SVAO.cpp:347-350) whose writes beyond the texture are
dropped, so the right and bottom guard band receive AO and stencil values and request SD rays; "AO 2" covers exactly
the visible size (SVAO.cpp:452-453: dims - 2 guardBand, not rounded up), so it leaves pass 1's AO outside it."""
import ctypes as C
import types
import weakref

import numpy as np
import pytest

from helpers import (ODD_FRAMES, PAD_ELEMENTS, SENTINEL, Canary, assert_canaries_intact, grade,  # noqa: F401
                     odd_frame, odd_frame_config, odd_second_pose, sentinel_array, to_oracle, visible_region)

pytestmark = pytest.mark.gpu

SHAPES = [f.name for f in ODD_FRAMES]
OUTPUTS = ("depth", "normals", "ao", "stencil", "ray_min", "ray_max", "sd")


@pytest.fixture(scope="module")
def ctx(oracle):
    """One device, one uploaded scene and its oracle twin for the module."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rsd.frame import Device, GpuScene
    from rsd.scenes import make_scene
    scene = make_scene("arcade_tiny")
    dev = Device(0)
    gscene = GpuScene(dev, scene)
    c = types.SimpleNamespace(torch=torch, O=oracle, scene=scene, dev=dev, gscene=gscene, base={},
                              osc=oracle.Scene(scene.positions, scene.indices, scene.flags, scene.alpha))
    c.bvh, c.tri_offset = gscene.export_bvh()
    yield c
    torch.cuda.synchronize()
    gscene.release()


def _renderer(ctx, f, **kw):
    """A renderer of the shape f over the module's scene whose seven output buffers are canary views."""
    from rsd import abi
    from rsd.frame import Renderer
    r = Renderer(ctx.scene, odd_frame_config(f, **kw), gpu_scene=ctx.gscene, dev=ctx.dev)
    r.canaries = {}
    for name in OUTPUTS:
        old = getattr(r, name)
        r.canaries[name] = Canary(ctx.torch, old.shape, old.dtype, old.device)
        setattr(r, name, r.canaries[name].view)
    r.ray_minmax = r.ray_min   # (only the key of the cached frame descriptor reads it)
    # ... and so is its busy-tile buffer (rsd_svao_params.tile_flags), zeroed once by its owner
    c = r.canaries["tile_flags"] = Canary(ctx.torch, r.tile_flags.shape, r.tile_flags.dtype, r.tile_flags.device)
    c.view.zero_()
    weakref.finalize(c.raw, abi.lib().rsd_svao_tile_flags_release, c.view.data_ptr())
    r.tile_flags = c.view
    r.svp.tile_flags = c.view.data_ptr()
    return r


def _intact(ctx, r, stage):
    assert_canaries_intact(ctx.torch, r.canaries, stage)


def _structs(ctx, r):
    O = ctx.O
    return (to_oracle(r.cam, O.Camera), to_oracle(r.vao, O.VAOData), to_oracle(r.sdp, O.SDParams),
            to_oracle(r.svp, O.SVAOParams))


def _upload(ctx, dst, a):
    a = np.array(a, order="C")   # a copy: the shared results are read-only
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(a.dtype)
    dst.copy_(ctx.torch.from_numpy(a.view(signed) if signed else a))


# ---- the stages on the GPU: every output pre-filled with the sentinel, the canaries checked after the call

def _gbuffer(ctx, r, cull=None):
    from rsd import abi
    for k in ("depth", "normals"):
        r.canaries[k].fill()
    cull = r.cfg.cull_mode if cull is None else cull
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    abi.check(abi.lib().rsd_gbuffer(r.gscene.h, C.byref(r.cam), r.cfg.fb_w, r.cfg.fb_h, cull, p(r.depth), p(r.normals),
                                    r.stream), "rsd_gbuffer")
    _intact(ctx, r, "G-buffer")
    g = r.numpy()
    return g["depth"], g["normals"]


def _pass1(ctx, r):
    for k in ("ao", "stencil", "ray_min", "ray_max"):
        r.canaries[k].fill()
    r.clear_intervals()
    _intact(ctx, r, "interval clear")
    r.pass1()
    _intact(ctx, r, "pass 1")
    g = r.numpy()
    return {k: g[k] for k in ("ao", "stencil", "ray_min", "ray_max")}


def _trace(ctx, r, p1=None):
    """The SD trace of the intervals p1 (default: the ones on the device) into a sentinel-filled map."""
    if p1 is not None:
        _upload(ctx, r.ray_min, p1["ray_min"])
        _upload(ctx, r.ray_max, p1["ray_max"])
    r.canaries["sd"].fill()
    r.sd_trace()
    _intact(ctx, r, "SD trace")
    return r.numpy()["sd"]


def _pass2(ctx, r, sd):
    """Pass 2 after a fresh pass 1 of this renderer (pass 1 flags the busy tiles pass 2 visits) over the map sd."""
    p1 = _pass1(ctx, r)
    _upload(ctx, r.sd, sd)
    r.pass2()
    _intact(ctx, r, "pass 2")
    return p1, r.numpy()["ao"]


# ---- the stages on the oracle, on the GPU's own inputs

def _oracle_pass1(ctx, r, depth, normals):
    O, cfg = ctx.O, r.cfg
    cam, vao, _, svp = _structs(ctx, r)
    ao = sentinel_array((cfg.fb_h, cfg.fb_w, 2) if cfg.dual_ao else (cfg.fb_h, cfg.fb_w), np.uint8)
    st = sentinel_array((cfg.fb_h, cfg.fb_w), O.stencil_dtype(cfg.num_directions))
    rmin, rmax = np.zeros((r.sd_h, r.sd_w), np.uint32), np.zeros((r.sd_h, r.sd_w), np.uint32)
    O.svao_clear(rmin, rmax)
    O.svao_pass1_into(cam, vao, svp, depth, normals, ao, st, rmin, rmax)
    return dict(ao=ao, stencil=st, ray_min=rmin, ray_max=rmax)


def _oracle_trace(ctx, r, depth, p1):
    O = ctx.O
    cam, _, sdp, _ = _structs(ctx, r)
    args = (cam, sdp, depth, p1["ray_min"], p1["ray_max"], r.sd_w, r.sd_h)
    if sdp.hit_order == 1:
        return O.sd_trace_ordered(ctx.osc, ctx.bvh, ctx.tri_offset, *args)
    if sdp.hit_order == 2:  # the wavefront order: librsd's pool bound from the tree depth (rsd.h)
        return O.sd_trace_wavefront(ctx.osc, ctx.bvh, ctx.tri_offset, min(208 - 3 * int(ctx.gscene.info.wide_depth), 160),
                                    *args)
    return O.sd_trace(ctx.osc, *args)


def _oracle_pass2(ctx, r, depth, normals, p1, sd):
    cam, vao, _, svp = _structs(ctx, r)
    return ctx.O.svao_pass2(cam, vao, svp, depth, normals, p1["stencil"], sd, p1["ao"])


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:  # bits, not values: a NaN equals itself, -0 is not +0
        got, want = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} elements differ, the first at {bad[:8].tolist()}")


def _same_pass1(got, want, what):
    for k in ("stencil", "ray_min", "ray_max", "ao"):
        _same(got[k], want[k], f"{what}: {k}")


def _base(ctx, name):
    """The shape's renderer with the default kernels' stages and the oracle's results on the GPU's own inputs, computed
    once per shape: G-buffer -> pass 1 -> SD trace of the GPU's intervals -> pass 2 of the GPU's stencil, AO and map."""
    if name not in ctx.base:
        r = _renderer(ctx, odd_frame(name))
        b = types.SimpleNamespace(r=r)
        b.depth, b.normals = _gbuffer(ctx, r)
        b.g1 = _pass1(ctx, r)
        b.o1 = _oracle_pass1(ctx, r, b.depth, b.normals)
        b.gsd = _trace(ctx, r)
        b.osd, b.stats = _oracle_trace(ctx, r, b.depth, b.g1)
        _, b.gao = _pass2(ctx, r, b.gsd)
        b.oao = _oracle_pass2(ctx, r, b.depth, b.normals, b.g1, b.gsd)
        for a in vars(b).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        ctx.base[name] = b
    return ctx.base[name]


# ---- G-buffer

@pytest.mark.parametrize("cull", [1, 0], ids=["back", "none"])
@pytest.mark.parametrize("name", SHAPES)
def test_gbuffer(ctx, name, cull):
    """rsd_gbuffer against oracle.gbuffer: depth bits and packed normals of every pixel, at widths that are no
    multiple of its block."""
    r = _renderer(ctx, odd_frame(name))
    depth, normals = _gbuffer(ctx, r, cull)
    z, n = ctx.O.gbuffer(ctx.osc, to_oracle(r.cam, ctx.O.Camera), r.cfg.fb_w, r.cfg.fb_h, cull)
    assert (z < r.cfg.far).sum() > z.size // 2, "the camera sees no geometry"
    _same(depth, z, "depth")
    _same(normals, n, "normals")


# ---- pass 1

@pytest.mark.parametrize("choice", [None, "generic"], ids=["default", "generic"])
@pytest.mark.parametrize("name", SHAPES)
def test_pass1(ctx, monkeypatch, name, choice):
    """AO, stencil, rayMin and rayMax of the whole buffers against oracle.svao_pass1 on the GPU's own G-buffer: the
    right / bottom guard band carries pass 1's values up to roundup32(visible), the left / top band and whatever lies
    beyond keep the sentinel."""
    b = _base(ctx, name)
    if choice is None:
        monkeypatch.delenv("RSD_PASS1", raising=False)
    else:
        monkeypatch.setenv("RSD_PASS1", choice)
    g1 = _pass1(ctx, b.r)
    cfg, g0 = b.r.cfg, b.r.cfg.guard_band
    if g0:  # the reference at the left / top band: no thread of the dispatch, the oracle's buffer keeps the sentinel
        assert (np.ascontiguousarray(b.o1["ao"][:g0]) == SENTINEL).all() and (b.o1["ao"][:, :g0] == SENTINEL).all()
    assert (b.o1["stencil"][visible_region(cfg)] != 0).any()
    _same_pass1(g1, b.o1, f"{name} {choice or 'default'} pass 1")


@pytest.mark.parametrize("name", SHAPES)
def test_busy_tiles(ctx, name):
    """The busy-tile buffer after the first pass 1 of a renderer (generation 0, stamp 1; svao_math.h tile_layout: T
    flag words, the two list counts, T list entries): flagged are exactly the 16 x 16 tiles with a stencilled VISIBLE
    pixel, and the list holds each of them once.  The padded dispatch runs up to 31 columns and rows past the visible
    region; a vote from there would flag a tile without visible pixels, alias the next tile row's first tile where
    roundup32(width) / 16 exceeds the tiles per row (odd_div4, no_guards, one_over), or land in the list counts."""
    from rsd import abi
    b = _base(ctx, name)
    r = _renderer(ctx, odd_frame(name))
    cfg = r.cfg
    _upload(ctx, r.depth, b.depth)
    _upload(ctx, r.normals, b.normals)
    _same_pass1(_pass1(ctx, r), b.o1, f"{name}: pass 1")
    tx, ty = -(-cfg.visible_w // 16), -(-cfg.visible_h // 32) * 2
    T = tx * ty
    assert abi.lib().rsd_svao_tile_count(cfg.fb_w, cfg.fb_h, cfg.guard_band) == 8 * T + 16 == r.tile_flags.numel()
    words = r.tile_flags.cpu().numpy().view(np.uint32)
    flags, count, listed = words[:T], words[T:T + 2], words[T + 4:]
    st = np.zeros((ty * 16, tx * 16), bool)
    st[:cfg.visible_h, :cfg.visible_w] = b.o1["stencil"][visible_region(cfg)] != 0
    want = np.flatnonzero(st.reshape(ty, 16, tx, 16).any(axis=(1, 3)))
    assert 0 < len(want) < T, "no tile or every tile is busy: the frame cannot show a wrong vote"
    assert np.array_equal(np.flatnonzero(flags), want) and (flags[want] == 1).all(), (np.flatnonzero(flags), want)
    assert (count[0], count[1]) == (len(want), 0), count
    assert np.array_equal(np.sort(listed[:len(want)]), want) and (listed[len(want):] == 0).all(), listed


@pytest.mark.parametrize("nd,dual", [(16, False), (32, True)], ids=["d16", "d32_dualao"])
def test_pass1_directions(ctx, nd, dual):
    """16 directions (R16Uint stencil) and 32 with dualAO (R32Uint stencil, RG8Unorm AO) at odd_div3."""
    base = _base(ctx, "odd_div3")
    r = _renderer(ctx, odd_frame("odd_div3"), num_directions=nd, dual_ao=dual)
    _upload(ctx, r.depth, base.depth)
    _upload(ctx, r.normals, base.normals)
    g1 = _pass1(ctx, r)
    o1 = _oracle_pass1(ctx, r, base.depth, base.normals)
    assert g1["stencil"].dtype.itemsize == nd // 8 and g1["ao"].shape[2:] == ((2,) if dual else ())
    assert (o1["stencil"][visible_region(r.cfg)] >> 8).any(), "no direction above the eighth requests a ray"
    _same_pass1(g1, o1, f"{nd} directions")


# ---- SD trace

_WALKS = {"default": {}, "split": {"RSD_TRACE_WALK": "split"}, "quad": {"RSD_TRACE_WALK": "quad"},
          "raster": {"RSD_TRACE_WALK": "raster"}, "twopass": {"RSD_SETUP_TWOPASS": "on"}}


@pytest.mark.parametrize("walk", list(_WALKS))
@pytest.mark.parametrize("name", SHAPES)
def test_sd_trace_walks(ctx, monkeypatch, name, walk):
    """The trace of the GPU's own intervals against oracle.sd_trace, every texel of the map: the default walk, the
    split, quad and raster walks and the two-pass setup, on SD maps whose sizes are no multiple of the 8 x 8 tile."""
    b = _base(ctx, name)
    for k in ("RSD_TRACE_WALK", "RSD_SETUP_TWOPASS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in _WALKS[walk].items():
        monkeypatch.setenv(k, v)
    assert b.stats[0] >= (30 if name == "tiny" else 300), "too few live SD rays"
    _same(_trace(ctx, b.r, b.g1), b.osd, f"{name} {walk}: SD map")


@pytest.mark.parametrize("order", [1, 2], ids=["traversal", "wavefront"])
@pytest.mark.parametrize("name", SHAPES)
def test_sd_trace_hit_orders(ctx, name, order):
    """The traversal and wavefront any-hit orders against the oracle's matching stream over librsd's own BVH
    (tests/test_gpu_hit_order.py's comparison)."""
    b = _base(ctx, name)
    r = b.r
    r.sdp.hit_order = order
    try:
        sd = _trace(ctx, r, b.g1)
        want, stats = _oracle_trace(ctx, r, b.depth, b.g1)
    finally:
        r.sdp.hit_order = 0
    assert stats[0] > 0
    _same(sd, want, f"{name} hit order {order}: SD map")


@pytest.mark.parametrize("N", [1, 2, 8, 16])
@pytest.mark.parametrize("name", ["odd_div3", "tiny"])
def test_sd_trace_sample_counts(ctx, name, N):
    """N = 1, 2, 8, 16 on the default walk (R32F, RG32F and two / four RGBA32F layers; max_count 16 with N = 16)."""
    base = _base(ctx, name)
    r = _renderer(ctx, odd_frame(name), N=N, max_count=max(8, N))
    _upload(ctx, r.depth, base.depth)
    _upload(ctx, r.normals, base.normals)
    g1 = _pass1(ctx, r)
    _same_pass1(g1, base.g1, "pass 1 does not depend on N")
    sd = _trace(ctx, r)
    want, stats = _oracle_trace(ctx, r, base.depth, g1)
    assert stats[0] > 0 and sd.shape == ((N + 3) // 4, r.sd_h, r.sd_w, min(N, 4))
    _same(sd, want, f"{name} N = {N}: SD map")


@pytest.mark.parametrize("name", SHAPES)
def test_clean_tiles_second_frame(ctx, name):
    """keep_clean_tiles(): two frames at two poses (tests/test_odd_geometry.py: the touched texels change both ways).
    The second SD map equals the oracle's trace of the second frame's own intervals, and the map of a renderer
    without clean tiles."""
    f = odd_frame(name)
    cln, ref = _renderer(ctx, f), _renderer(ctx, f)
    cln.keep_clean_tiles()
    touched = []
    for pose in (None, odd_second_pose(ctx.scene)):
        for r in (cln, ref):
            if pose is not None:
                r.set_pose(*pose)
            _gbuffer(ctx, r)
            for k in ("ao", "stencil", "ray_min", "ray_max") + (("sd",) if pose is None else ()):
                r.canaries[k].fill()   # (the second trace may skip the tiles the first left clean)
            r.frame()
            _intact(ctx, r, "frame")
        touched.append(cln.numpy()["ray_max"] != 0)
    assert (touched[0] & ~touched[1]).any() and (touched[1] & ~touched[0]).any()
    g, gr = cln.numpy(), ref.numpy()
    want, stats = _oracle_trace(ctx, cln, g["depth"], g)
    assert stats[0] > 0
    _same(g["sd"], want, f"{name}: second SD map with clean tiles against the oracle")
    _same(g["sd"], gr["sd"], f"{name}: second SD map with and without clean tiles")
    _same(g["ao"], gr["ao"], f"{name}: second AO with and without clean tiles")


# ---- pass 2

_PASS2 = {"default": {}, "generic": {"RSD_PASS2": "generic"}, "list_off": {"RSD_PASS2_LIST": "off"},
          "loop_off": {"RSD_PASS2_LOOP": "off"}, "no_tile_flags": {}}


@pytest.mark.parametrize("variant", list(_PASS2))
@pytest.mark.parametrize("name", SHAPES)
def test_pass2(ctx, monkeypatch, name, variant):
    """The AO of the whole buffer against oracle.svao_pass2 on the GPU's own stencil, pass-1 AO and SD map: the
    busy-tile list in the resident loop (default), the generic kernel, the flag grid, one workgroup per listed tile,
    and no tile flags at all.  Outside the visible region pass 2 leaves pass 1's AO (and the sentinel) unchanged."""
    from rsd import abi
    b = _base(ctx, name)
    r = b.r
    for k in ("RSD_PASS2", "RSD_PASS2_LIST", "RSD_PASS2_LOOP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in _PASS2[variant].items():
        monkeypatch.setenv(k, v)
    svp = r.svp
    if variant == "no_tile_flags":
        r.svp = abi.SVAOParams.from_buffer_copy(svp)
        r.svp.tile_flags = None
    try:
        p1, ao = _pass2(ctx, r, b.gsd)
    finally:
        r.svp = svp
    _same_pass1(p1, b.g1, "the pass 1 before it")
    _same(ao, b.oao, f"{name} {variant}: AO")
    outside = np.ones(ao.shape[:2], bool)
    outside[visible_region(r.cfg)] = False
    assert np.array_equal(ao[outside], b.g1["ao"][outside]), "pass 2 wrote outside the visible region"
    assert not np.array_equal(ao, b.g1["ao"]), "pass 2 changed nothing"


# ---- the frame in one call

@pytest.mark.parametrize("name", SHAPES)
def test_one_call_frame(ctx, name):
    """rsd_svao_frame (Renderer.frame()) gives the five buffers of the separate stages: AO, stencil, rayMin, rayMax
    and the SD map."""
    b = _base(ctx, name)
    r = _renderer(ctx, odd_frame(name))
    _upload(ctx, r.depth, b.depth)
    _upload(ctx, r.normals, b.normals)
    for k in ("ao", "stencil", "ray_min", "ray_max", "sd"):
        r.canaries[k].fill()
    r.frame()
    _intact(ctx, r, "rsd_svao_frame")
    g = r.numpy()
    _same_pass1(dict(g, ao=b.g1["ao"]), b.g1, f"{name}: one call")
    _same(g["sd"], b.gsd, f"{name}: one call: SD map")
    _same(g["ao"], b.gao, f"{name}: one call: AO")
    _same(g["ao"], b.oao, f"{name}: one call: AO against the oracle")


# ---- row splits

def _pieces(end, step):
    """[0, step), [step, 2 step), ... with the last piece ending at `end`."""
    cuts = list(range(0, end, step)) + [end]
    return list(zip(cuts[:-1], cuts[1:]))


def _rows_untouched(before, after, lo, hi, what):
    keep = np.ones(before.shape[0], bool)
    keep[lo:hi] = False
    assert np.array_equal(before[keep], after[keep]), f"{what}: rows outside [{lo}, {hi}) changed"


@pytest.mark.parametrize("name", SHAPES)
def test_row_splits(ctx, name):
    """rsd_svao_pass1_rows / rsd_svao_pass2_rows at every legal boundary (multiples of 32 of the visible rows, the
    last piece ending the frame) and rsd_sd_trace_rows at every multiple of 8, the pieces in sequence: together the
    bits of the whole-frame calls, and no piece changes a row that is not its own.  A boundary off the grid is
    refused."""
    from rsd import abi
    b = _base(ctx, name)
    r = _renderer(ctx, odd_frame(name))
    cfg = r.cfg
    g0, vh, H = cfg.guard_band, cfg.visible_h, cfg.fb_h
    px_pieces, sd_pieces = _pieces(vh, 32), _pieces(r.sd_h, 8)
    if name == "tiny":
        assert px_pieces == [(0, vh)]
    else:
        assert len(px_pieces) >= 2 and len(sd_pieces) >= 4
    for call, rows in ((r.pass1_rows, (0, 8)), (r.pass1_rows, (16, vh)), (r.pass2_rows, (0, 8)),
                       (r.pass2_rows, (16, vh)), (r.sd_trace_rows, (0, 4)), (r.sd_trace_rows, (4, r.sd_h))):
        with pytest.raises(abi.RsdError) as e:
            call(rows)
        assert e.value.status == abi.ERR_INVALID_ARG
    _upload(ctx, r.depth, b.depth)
    _upload(ctx, r.normals, b.normals)

    # pass 1: a piece stores the rows of its 32-row groups (the last group runs to roundup32 or the buffer's end)
    for k in ("ao", "stencil", "ray_min", "ray_max"):
        r.canaries[k].fill()
    r.clear_intervals()
    for r0, r1 in px_pieces:
        before = r.numpy()
        r.pass1_rows((r0, r1))
        _intact(ctx, r, f"pass 1 rows {r0}-{r1}")
        after = r.numpy()
        for k in ("ao", "stencil"):
            _rows_untouched(before[k], after[k], g0 + r0, min(g0 + (r1 + 31) // 32 * 32, H), f"pass 1 rows {r0}-{r1}: {k}")
    _same_pass1(r.numpy(), b.g1, f"{name}: pass 1 in pieces")

    # SD trace
    r.canaries["sd"].fill()
    for r0, r1 in sd_pieces:
        before = r.numpy()
        r.sd_trace_rows((r0, r1))
        _intact(ctx, r, f"SD rows {r0}-{r1}")
        after = r.numpy()
        _rows_untouched(before["sd"].transpose(1, 0, 2, 3), after["sd"].transpose(1, 0, 2, 3), r0, r1, f"SD rows {r0}-{r1}")
        assert np.array_equal(before["ray_min"], after["ray_min"]) and np.array_equal(before["ray_max"], after["ray_max"])
    _same(r.numpy()["sd"], b.gsd, f"{name}: SD trace in pieces")

    # pass 2: a piece refines its visible rows only
    for r0, r1 in px_pieces:
        before = r.numpy()
        r.pass2_rows((r0, r1))
        _intact(ctx, r, f"pass 2 rows {r0}-{r1}")
        _rows_untouched(before["ao"], r.numpy()["ao"], g0 + r0, g0 + min(r1, vh), f"pass 2 rows {r0}-{r1}")
    _same(r.numpy()["ao"], b.gao, f"{name}: pass 2 in pieces")


# ---- fast numerics

@pytest.mark.parametrize("name", ["odd_div3", "no_guards"])
def test_fast_numerics(ctx, name):
    """The product's default arithmetic on the odd frames, graded by helpers.grade against the exact oracle
    (BASELINE.md section 4's AO tolerance and decision fractions); the canaries hold."""
    r = _renderer(ctx, odd_frame(name), numerics="fast")
    _gbuffer(ctx, r)
    for k in ("ao", "stencil", "sd"):
        r.canaries[k].fill()
    frame = grade(ctx.O, r, ctx.scene, f"odd_geometry_{name}")
    print(name, frame)
    _intact(ctx, r, "fast frame")
