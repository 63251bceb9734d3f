"""The shapes of tests/test_gpu_odd_passes.py can show a fault (CPU: the checkers and the oracle alone).

tests/test_gpu_odd_passes.py runs the ray and raster passes outside the SVAO frame -- rsd_gbuffer_raster,
rsd_gbuffer_world, rsd_depth_peel, rsd_rtao, rsd_rtao_pack, rsd_sd_raster, rsd_hbao, rsd_temporal_depth_peel -- and
the SVAO leftovers (the ray-traced pass 2, the interleaved band calls) at frames off their tile grids, into canary
buffers.  A green comparison there means nothing on a frame where every pixel misses or no texel is darkened, so this
module asserts on the references alone, as tests/test_odd_geometry.py does for the SVAO frame, that every shape
reaches what it is meant to reach.  These are conditions on the inputs (helpers.ODD_PASS_CAMERA and its neighbours
were chosen to meet them), not measurements: an input that misses one is replaced, the condition stays.

It also shows, again on the references alone, that the shapes are sensitive to the mutants the GPU tests name in their
docstrings (test_mutants_*): a row stride taken from the padded width, a grid that is not rounded up, a scissor
that is off by one, a ray-pipeline grid that stops at the visible edge, a band that counts its 32-row groups from
the frame's first row."""
import numpy as np
import pytest

import depth_peel_checker as DP
import hbao_checker as HB
import rtao_checker as RT
import sd_raster_checker as SR
import temporal_peel_checker as TP
from helpers import (BLOCK_SHAPES, HBAO_EMPTY_SCISSOR, HBAO_ONE_TEXEL_SCISSOR, HBAO_SHAPES, ODD_FRAMES, ODD_PASS_FAR,
                     ODD_PASS_RTAO_MAX_T, ODD_PASS_SD_DIVISORS, ODD_PASS_SD_RADIUS, ODD_PASS_SD_SAMPLES, ODD_SD_SIZES,
                     PIXEL_SHAPES, SENTINEL, TEMPORAL_PEEL_SHAPES, band_counts, band_rows, hbao_odd_input,
                     odd_frame_config, odd_pass_case, oracle_vao, restride, right_bottom_guard, roundup, shape_id,
                     to_oracle, visible_region)

KINDS = ["opaque", "alpha"]
# Whether the ray-pipeline grid (ray_pipeline = 1: from the guard band to the right / bottom edge) changes an AO byte
# outside the visible region.  Every shape with a guard band does, `tiny` (3 pixels) and `one_over` (1 pixel)
# included; `no_guards` has no guard band, so it has no pixel there: on that shape the GPU test cannot tell the two
# grids apart, and says so here by name
RAY_PIPELINE_REACHES_THE_GUARD_BAND = {"odd_div3": True, "odd_div4": True, "no_guards": False, "tiny": True,
                                       "one_over": True}


def _big(size):
    return size[0] >= 8 and size[1] >= 8


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


def test_the_shape_lists():
    """The lists themselves: the sizes around the 8 x 8 tile and the 64 x 4 block, the HBAO scissors."""
    assert PIXEL_SHAPES == [(1, 1), (7, 3), (8, 8), (9, 9), (65, 17)]
    assert [w * h for w, h in PIXEL_SHAPES] == [1, 21, 64, 81, 1105]
    assert BLOCK_SHAPES == [(1, 1), (3, 2), (5, 7), (256, 16), (257, 17)]
    assert [((w + 3) // 4, (h + 3) // 4) for w, h in BLOCK_SHAPES] == [(1, 1), (1, 1), (2, 2), (64, 4), (65, 5)]
    assert TEMPORAL_PEEL_SHAPES == BLOCK_SHAPES + [(64, 4), (65, 5)]
    # guard band 0 everywhere; guard band 8 (two texels a side) leaves a texel only on the 65 x 5 layers
    assert HBAO_SHAPES == [(w, h, 0) for w, h in BLOCK_SHAPES[:4]] + [(257, 17, 0), (257, 17, 8)]
    scissor = lambda w, h, g: ((w + 3) // 4 - 2 * (g // 4), (h + 3) // 4 - 2 * (g // 4))  # noqa: E731
    assert scissor(*HBAO_EMPTY_SCISSOR) == (2, -2) and scissor(*HBAO_ONE_TEXEL_SCISSOR) == (1, 1)
    assert HB.scissored_texels(*HBAO_EMPTY_SCISSOR) == 16 * 10 * 6
    assert HB.scissored_texels(*HBAO_ONE_TEXEL_SCISSOR) == 16 * (11 * 11 - 1)


# ---------------------------------------------------------------------------------- the 8 x 8-tile kernels

_tile = {}


def tile_frame(oracle, dp, kind, size, cull):
    """The oracle's raster G-buffer of the case and the depth-peel checker's second layers (computed once)."""
    key = (kind, size, cull)
    if key not in _tile:
        c = odd_pass_case(oracle, DP, kind, size)
        d, nw = oracle.gbuffer_raster(c.osc, c.ocam, size[0], size[1], cull)
        z = oracle.linearize_depth(d, c.ocam.nearZ, c.ocam.farZ)
        second = {pc: DP.peel(oracle, dp, c, pc, z, 0.5, 1, width=size[0], height=size[1]) for pc in (0, 1, 2)}
        _tile[key] = dict(case=c, depth=d, normal_w=nw, z=z, second=second)
    return _tile[key]


@pytest.mark.parametrize("cull", [0, 1], ids=["none", "back"])
@pytest.mark.parametrize("size", PIXEL_SHAPES, ids=shape_id)
@pytest.mark.parametrize("kind", KINDS)
def test_gbuffer_hits_and_misses(oracle, dp, kind, size, cull):
    """From 8 x 8 on at least 5 % of the pixels hit and 5 % miss (farZ = ODD_PASS_FAR); below, a pixel hits."""
    f = tile_frame(oracle, dp, kind, size, cull)
    hit = f["depth"] < 1.0
    print(kind, size, cull, "hit", float(hit.mean()))
    assert f["case"].ocam.farZ == ODD_PASS_FAR
    assert hit.any()
    if _big(size):
        assert hit.mean() >= 0.05 and (~hit).mean() >= 0.05


@pytest.mark.parametrize("size", [s for s in PIXEL_SHAPES if _big(s)], ids=shape_id)
@pytest.mark.parametrize("kind", KINDS)
def test_depth_peel_has_a_second_layer(oracle, dp, kind, size):
    """At separation 0.5, with every cull mode of the peel, at least 5 % of the hit pixels get a second layer."""
    for gcull in (0, 1):
        f = tile_frame(oracle, dp, kind, size, gcull)
        hit = f["depth"] < 1.0
        for pc, layer in f["second"].items():
            share = float(((layer < np.float32(ODD_PASS_FAR)) & hit).sum() / hit.sum())
            print(kind, size, "gbuffer cull", gcull, "peel cull", pc, "second layer on", share, "of the hits")
            assert share >= 0.05


def _rtao_rays(oracle, rt, size, frame):
    c = odd_pass_case(oracle, RT, "opaque", size)
    pw = RT.posw(oracle, rt, c, 1, width=size[0], height=size[1])
    _, nw = oracle.gbuffer_raster(c.osc, c.ocam, size[0], size[1], 1)
    orig, d = RT.origins(rt, pw, nw, 0.01), RT.dirs(rt, pw, nw, frame)
    return pw, RT.trace(oracle, rt, c.osc, c.has_alpha, orig, d, ODD_PASS_RTAO_MAX_T)[..., 0]


@pytest.mark.parametrize("frame", [0, 7])
@pytest.mark.parametrize("size", [s for s in PIXEL_SHAPES if _big(s)], ids=shape_id)
def test_rtao_rays_hit_and_miss(oracle, rt, size, frame):
    """spp = 1, maxTHit = ODD_PASS_RTAO_MAX_T: at least 5 % of the valid pixels have a ray that hits, 5 % one that
    misses."""
    pw, t = _rtao_rays(oracle, rt, size, frame)
    valid = pw[..., 3] != 0
    share = float((t > 0)[valid].mean())
    print(size, frame, "valid", int(valid.sum()), "hit share", share)
    assert share >= 0.05 and 1.0 - share >= 0.05


def sd_raster_frames(oracle, sr):
    """(size, divisor, case, oracle frame) of every raster SD map the GPU test runs: PIXEL_SHAPES x divisors."""
    for size in PIXEL_SHAPES:
        case = SR.Case(oracle, SR.BASE["kind"], size)
        for divisor in ODD_PASS_SD_DIVISORS:
            yield size, divisor, case, SR.oracle_frame(oracle, case, divisor, ODD_PASS_SD_RADIUS, 4, SR.BASE["cull"])


def test_raster_sd_stores_samples_behind_the_first_layer(oracle, sr):
    """sd_raster_checker's base case on the derived maps: below a tile, exactly a tile, one over; every map of at
    least 64 texels holds a texel with a stored sample, at N = 1, 4, 16.  Of the maps with a divisor above 1, 33 x 9
    and 5 x 5 (divisor 2) are no multiple of it on either axis, 22 x 6 (divisor 3) on its width only, 4 x 2 and
    3 x 3 (from 7 x 3 and 9 x 9) are multiples: the shapes are the issue's, the ragged ones are named here."""
    sizes = set()
    for size, divisor, case, fr in sd_raster_frames(oracle, sr):
        assert (fr.sd_w, fr.sd_h) == (-(-size[0] // divisor), -(-size[1] // divisor))
        sizes.add((fr.sd_w, fr.sd_h))
        for N in ODD_PASS_SD_SAMPLES:
            prm = SR.params(N=N, alpha=SR.BASE["alpha"], cull=SR.BASE["cull"], use_stencil=True)
            m, cnt = SR.raster(oracle, sr, case, prm, fr.depth, fr.sd_w, fr.sd_h, fr.rmin, fr.rmax)
            behind = int((m < 1.0).any(axis=(0, 3)).sum())
            print(size, divisor, N, (fr.sd_w, fr.sd_h), "texels with a stored sample", behind)
            assert m.shape == ((N + 3) // 4, fr.sd_h, fr.sd_w, min(N, 4))
            if fr.sd_w * fr.sd_h >= 64:
                assert behind >= 1
    assert {(8, 8), (9, 9), (7, 3), (65, 17), (33, 9), (22, 6), (5, 5), (3, 3)} <= sizes
    assert 33 % 2 and 9 % 2 and 5 % 2 and 22 % 3 and not 6 % 3 and not 4 % 2 and not 3 % 3


# ---------------------------------------------------------------------------------- the 64 x 4-block kernels

@pytest.mark.parametrize("shape", HBAO_SHAPES + [HBAO_EMPTY_SCISSOR, HBAO_ONE_TEXEL_SCISSOR], ids=shape_id)
def test_hbao_answers_are_not_the_sentinel(hb, shape):
    """Inside the scissor no answer of the checker is the canary's sentinel pair, in both depth modes and at both
    exponents, so a sentinel left there can only be a texel that was not written; from 2 x 2 layers on a texel is
    darkened; the scissored count is the one the sizes give."""
    W, H, guard = shape
    s, radius = hbao_odd_input(HB, W, H)
    for mode in (HB.SINGLE, HB.DUAL):
        for exponent in HB.EXPONENTS:
            out, flags = HB.hbao(hb, s["layers"], s["layers2"], s["normal_w"], s["cam"], radius=radius,
                                 exponent=exponent, depth_mode=mode, guard_band=guard, fill=SENTINEL)
            inside = (flags & HB.SCISSORED) == 0
            assert int((~inside).sum()) == HB.scissored_texels(W, H, guard)
            assert (out[~inside] == SENTINEL).all()
            assert not (out[inside] == SENTINEL).all(-1).any(), (shape, mode, exponent)
            if shape[:2] in BLOCK_SHAPES[2:]:
                assert (out[inside] < 255).any(), (shape, mode, exponent)
    if shape == HBAO_EMPTY_SCISSOR:
        assert not inside.any()
    if shape == HBAO_ONE_TEXEL_SCISSOR:
        assert inside.sum(axis=(1, 2)).tolist() == [1] * 16 and inside[:, 5, 5].all()


def test_hbao_layers_of_the_3x2_frame(hb):
    """3 x 2: every layer is one texel; layer 4 dy + dx holds pixel (dx, dy), so six layers hold a pixel of the image
    and ten a texel beyond it (flag RAGGED), which rsd_hbao shades like any other."""
    s, radius = hbao_odd_input(HB, 3, 2)
    out, flags = HB.hbao(hb, s["layers"], None, s["normal_w"], s["cam"], radius=radius, fill=SENTINEL)
    assert out.shape == (16, 1, 1, 2)
    holds = [layer for layer in range(16) if layer % 4 < 3 and layer // 4 < 2]
    assert holds == [0, 1, 2, 4, 5, 6]
    assert np.flatnonzero((flags[:, 0, 0] & HB.RAGGED) == 0).tolist() == holds
    assert not (out == SENTINEL).all(-1).any()


@pytest.mark.parametrize("pose", TP.POSES)
@pytest.mark.parametrize("size", TEMPORAL_PEEL_SHAPES, ids=shape_id)
def test_temporal_peel_moves_and_keeps(tp, size, pose):
    """At every separation and iteration count of the checker's lists the output holds reprojected texels and
    texels left at the first layer (no information: the pass's cleared value), except on the 1 x 1 frame; a first
    frame (a history of zeros) leaves every texel there."""
    s = TP.synthetic(tp, *size, pose)
    for sep in TP.SEPARATIONS:
        for iterations in TP.ITERATIONS:
            out, flags = TP.peel(tp, s["z"], s["prev2"], s["cam"], s["c2p"], s["p2c"], sep, iterations)
            moved = TP.bits(out) != TP.bits(s["z"])
            assert (flags & TP.CLIP_CAP == 0).all()
            if size != (1, 1):
                assert moved.any() and (~moved).any(), (size, pose, sep, iterations)
    first, _ = TP.peel(tp, s["z"], np.zeros_like(s["z"]), s["cam"], s["c2p"], s["p2c"], 0.5, 32)
    assert np.array_equal(TP.bits(first), TP.bits(s["z"]))


# ---------------------------------------------------------------------------------- the SVAO leftovers

_rt = {}


def raytraced_frame(O, f):
    """The oracle's G-buffer and pass 1 of the odd frame f in the Raytraced secondary mode, and its ray-traced pass 2
    with both grids (computed once)."""
    if f.name not in _rt:
        from rsd import abi
        from rsd.frame import svao_params
        from rsd.scenes import make_scene
        cfg = odd_frame_config(f, secondary=abi.DEPTH_RAYTRACED, numerics="exact")
        W, H = cfg.fb_w, cfg.fb_h
        s = make_scene("arcade_tiny")
        cam = O.camera_look_at(s.camera["pos"], s.camera["target"], s.camera["up"], focal_length=cfg.focal_length,
                               frame_height=cfg.frame_height, aspect=float(np.float32(W) / np.float32(H)),
                               near=cfg.near, far=cfg.far)
        osc = O.Scene(s.positions, s.indices, s.flags)
        z, n = O.gbuffer(osc, cam, W, H, cfg.cull_mode)
        vao, sd_w, sd_h = oracle_vao(O, W, H, cfg.divisor, 0, cfg.radius, cfg.exponent, cfg.thickness)
        svp = to_oracle(svao_params(cfg), O.SVAOParams)
        ao1, st, _, _ = O.svao_pass1(cam, vao, svp, z, n, sd_w, sd_h)
        ao = {rp: O.svao_pass2_raytraced(osc, cam, vao, svp, z, n, st, ao1, cull=cfg.cull_mode, ray_pipeline=rp)
              for rp in (0, 1)}
        _rt[f.name] = dict(cfg=cfg, ao1=ao1, stencil=st, ao=ao)
    return _rt[f.name]


@pytest.mark.parametrize("f", ODD_FRAMES, ids=[f.name for f in ODD_FRAMES])
def test_raytraced_pass2_changes_the_frame(oracle, f):
    """oracle.svao_pass2_raytraced changes an AO byte with either grid; ray_pipeline = 0 changes none outside the
    visible region; ray_pipeline = 1 changes one in the right / bottom guard band on the shapes
    RAY_PIPELINE_REACHES_THE_GUARD_BAND names, and on the others -- named there too -- it cannot."""
    o = raytraced_frame(oracle, f)
    cfg = o["cfg"]
    outside = np.ones((cfg.fb_h, cfg.fb_w), bool)
    outside[visible_region(cfg)] = False
    for rp in (0, 1):
        assert (o["ao"][rp] != o["ao1"]).any(), rp
    assert not (o["ao"][0] != o["ao1"])[outside].any()
    changed = (o["ao"][1] != o["ao1"]) & outside
    assert not (changed & ~right_bottom_guard(cfg)).any(), "a change left of or above the guard band"
    print(f.name, "AO bytes changed in the guard band with the ray-pipeline grid:", int(changed.sum()),
          "stencilled there:", int(((o["stencil"] != 0) & outside).sum()))
    assert set(RAY_PIPELINE_REACHES_THE_GUARD_BAND) == {g.name for g in ODD_FRAMES}
    assert bool(changed.any()) == RAY_PIPELINE_REACHES_THE_GUARD_BAND[f.name], f.name
    if RAY_PIPELINE_REACHES_THE_GUARD_BAND[f.name]:
        # the mutant "the ray-pipeline grid stops at the visible edge" is the other grid's image
        assert not np.array_equal(o["ao"][0], o["ao"][1])


@pytest.mark.parametrize("f", ODD_FRAMES, ids=[f.name for f in ODD_FRAMES])
def test_band_rows(f):
    """The 32-row groups and 8-row SD tile rows of each odd frame, dealt to 2, 3 and (groups + 1) bands: the last
    count leaves a band without a group on every shape, `tiny` has an empty band at every count (one group; two
    tile rows), and `odd_div3` none at 2 bands.  The bands partition the groups and the tile rows."""
    sd_h = ODD_SD_SIZES[f.name][1]
    groups, tiles = -(-f.visible_h // 32), -(-sd_h // 8)
    counts = band_counts(f)
    assert counts == [2, 3, groups + 1]
    for B in counts:
        rows = band_rows(f, B)
        print(f.name, "bands", B, rows)
        assert sorted(g for gs, _ in rows for g in gs) == list(range(groups))
        assert sorted(t for _, ts in rows for t in ts) == list(range(tiles))
        if f.name == "tiny":
            assert any(not gs for gs, _ in rows)
    assert not band_rows(f, groups + 1)[groups][0]
    if f.name == "tiny":
        assert (groups, tiles) == (1, 2) and band_rows(f, 3)[2] == ([], [])
    if f.name == "odd_div3":
        assert all(gs and ts for gs, ts in band_rows(f, 2))
    # the mutant "groups counted from the frame's first row": frame row y goes to band (y // 32) % B in place of
    # ((y - guard) // 32) % B.  It deals a band other rows on every shape with a guard band whose visible rows cross
    # a multiple of 32 of the frame; `tiny` (rows 3 to 14, one group) and `no_guards` cannot tell
    ys = np.arange(f.guard, f.guard + f.visible_h)
    for B in (2, 3):
        right, mutant = ((ys - f.guard) // 32) % B, (ys // 32) % B
        differ = [b for b in range(B) if not np.array_equal(right == b, mutant == b)]
        print(f.name, "bands", B, "bands whose rows the mutant changes:", differ)
        assert bool(differ) == (f.name in ("odd_div3", "odd_div4", "one_over")), (f.name, B)


# ---------------------------------------------------------------------------------- mutants, on the references alone

@pytest.mark.parametrize("kind", KINDS)
def test_mutants_of_the_tile_kernels_show(oracle, dp, rt, kind):
    """A row stride of roundup8(W) in place of W changes the expected depth, normal, posW and second layer on every
    PIXEL_SHAPES frame of more than one row whose width is no multiple of 8 (the RTAO ray log and the raster SD map
    have tests of their own below).  On 8 x 8 the stride is right by construction and on 1 x 1
    there is one element; there the canaries and the `<` of the bounds test are what a fault shows on: a lane at
    x == W or y == H stores one element past its row or buffer, into the next row (a differing pixel) or the canary."""
    for size in PIXEL_SHAPES:
        W, H = size
        f = tile_frame(oracle, dp, kind, size, 1)
        if W % 8 == 0 or H == 1:
            continue
        c = f["case"]
        images = {"depth": f["depth"], "normal": f["normal_w"], "second layer": f["second"][1],
                  "posW": RT.posw(oracle, rt, c, 1, width=W, height=H)}
        for name, im in images.items():
            assert not np.array_equal(restride(im, roundup(W, 8)), im), (size, name)


def test_mutant_of_the_rtao_ray_log_shows(oracle, dp, rt):
    """The checker's ray log of the 9 x 9 frame at spp = 4 (the float64 directions of the generator rounded to
    float32, traced by the checker; 16 floats per pixel): the four rays of every valid pixel differ from each other,
    and a log packed with a pixel stride of 4 floats -- ray i of pixel o at entry o + i, so that entry o ends up
    holding some ray of a pixel from o - 3 to o -- is not the expected log, whichever of those rays lands last."""
    import ctypes as C

    from rsd import abi
    size, frame = (9, 9), 3
    f = tile_frame(oracle, dp, "opaque", size, 1)
    c, nw = f["case"], f["normal_w"]
    pw = RT.posw(oracle, rt, c, 1, width=9, height=9)
    prm, tmax = abi.RTAOParams(max_t_hit=ODD_PASS_RTAO_MAX_T, spp=4, apply_exponential_falloff=True), C.c_float()
    abi.check(abi.lib().rsd_rtao_ray_t_max(C.byref(prm), C.byref(tmax)), "rsd_rtao_ray_t_max")
    valid = pw[..., 3] != 0
    d = np.zeros((9, 9, 4, 4), np.float32)
    d[..., :3] = np.nan_to_num(RT.dirs_float64(nw, frame, 4)).astype(np.float32)
    t = RT.trace(oracle, rt, c.osc, c.has_alpha, RT.origins(rt, pw, nw, prm.normal_scale), d, tmax.value)
    log = np.where(valid[..., None, None], np.concatenate([d[..., :3], t[..., None]], -1), 0).astype(np.float32)
    assert valid.sum() >= 20 and (t > 0)[valid].any() and (t == 0)[valid].any()
    for i in range(4):
        for j in range(i):
            assert (log[:, :, i] != log[:, :, j]).any(-1)[valid].all(), (i, j)
    want = log.reshape(-1, 4)  # the expected entries: spp o + i
    rays = log.reshape(81, 4, 4)
    # what the mutant can leave in entry o: ray o - p of a pixel p from o - 3 to o (from entry 5 on none of them is
    # the expected ray o % 4 of pixel o // 4 by position)
    entries = [o for o in range(5, 81) if valid.reshape(-1)[o - 3:o + 1].all()]
    wrong = [o for o in entries if not any(np.array_equal(want[o], rays[p, o - p]) for p in range(o - 3, o + 1))]
    print("ray log at 9 x 9: entries of the mutant's reach", len(entries), "that no candidate ray matches", len(wrong))
    assert len(entries) >= 10 and len(wrong) == len(entries)


def test_mutants_of_the_raster_sd_show(oracle, sr):
    """The raster SD checker's maps at N = 16 (four layers of RGBA32F): on every map of at least 64 texels whose
    width is no multiple of 8 -- 9 x 9, 65 x 17, 33 x 9, 22 x 6 -- a row stride of roundup8(w) changes a layer, and a
    layer stride of roundup8(w) * roundup8(h) texels moves layers 1 to 3 (each of them differs from what the mutant
    leaves there) and runs past the map's end (into the canary)."""
    seen = set()
    for size, divisor, case, fr in sd_raster_frames(oracle, sr):
        w, h = fr.sd_w, fr.sd_h
        if w * h < 64 or w % 8 == 0:
            continue
        seen.add((w, h))
        prm = SR.params(N=16, alpha=SR.BASE["alpha"], cull=SR.BASE["cull"], use_stencil=True)
        m, _ = SR.raster(oracle, sr, case, prm, fr.depth, w, h, fr.rmin, fr.rmax)
        assert m.shape == (4, h, w, 4)
        assert any(not np.array_equal(restride(m[layer], roundup(w, 8)), m[layer]) for layer in range(4)), (w, h)
        plane = roundup(w, 8) * roundup(h, 8)
        moved = restride(m.reshape(4, h * w, 4), plane)
        assert 4 * plane > 4 * h * w  # the last layer's end lies past the buffer
        for layer in (1, 2, 3):
            assert not np.array_equal(moved[layer], m.reshape(4, h * w, 4)[layer]), (w, h, layer)
    assert seen == {(9, 9), (65, 17), (33, 9), (22, 6)}


def test_mutants_of_the_block_kernels_show(hb, tp):
    """rsd_hbao: a layer row stride of roundup64(qw) changes the expected layers wherever qw is no multiple of 64
    and the layer has more than one row; a scissor test of `<=` in place of `<` would write a texel that the
    expected buffer keeps at the sentinel, and the unscissored answer there is not the sentinel.
    rsd_temporal_depth_peel: a row stride of roundup64(W) changes the expected layer on every frame of more than one
    row whose width is no multiple of 64."""
    for W, H, guard in HBAO_SHAPES + [HBAO_ONE_TEXEL_SCISSOR]:
        s, radius = hbao_odd_input(HB, W, H)
        out, flags = HB.hbao(hb, s["layers"], None, s["normal_w"], s["cam"], radius=radius, guard_band=guard,
                             fill=SENTINEL)
        qh, qw = out.shape[1:3]
        if qw % 64 and qh > 1:
            assert not np.array_equal(restride(out[0], roundup(qw, 64)), out[0]), (W, H, guard)
        if guard:
            free, _ = HB.hbao(hb, s["layers"], None, s["normal_w"], s["cam"], radius=radius, guard_band=0, fill=SENTINEL)
            g = guard // 4
            assert not (free[:, g:qh - g, qw - g] == SENTINEL).all(-1).any()  # the column a `<=` would add
            assert (out[:, g:qh - g, qw - g] == SENTINEL).all()
    for size in TEMPORAL_PEEL_SHAPES:
        if size[0] % 64 == 0 or size[1] == 1:
            continue
        s = TP.synthetic(tp, *size, "step")
        out, _ = TP.peel(tp, s["z"], s["prev2"], s["cam"], s["c2p"], s["p2c"], 0.5, 32)
        assert not np.array_equal(restride(out, roundup(size[0], 64)), out), size


def test_mutant_of_the_pack_kernel_shows():
    """rsd_rtao_pack with a grid of count / 256 blocks (not rounded up) leaves the last count % 256 elements at the
    sentinel: the expected bytes there are not the sentinel's, at every count of the GPU test that is no multiple
    of 256."""
    from helpers import PACK_COUNTS, pack_expected, pack_inputs
    for count in PACK_COUNTS:
        amb, dist = pack_inputs(count)
        a8, d16 = pack_expected(amb, dist)
        tail = slice(count // 256 * 256, count)
        if count % 256:
            assert (a8[tail] != SENTINEL).any() and (d16[tail] != SENTINEL * 0x0101).any()
