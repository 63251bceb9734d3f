"""CPU: the alpha test at its texture, LOD and contract edges -- the oracle against tests/alpha_checker.py on the hit
tuples of the very frames that tests/test_gpu_alpha_edges.py renders (tests/alpha_edge_scenes.py), and the proof that
those frames reach every edge the checker knows.

Hit tuples.  LOD 0 (the G-buffers, the depth peel, the raster SD map, RTAO, pass 2 Raytraced): the card each primary
ray of the 192 x 128 frame meets, from tests/mvec_checker.py on the scene with opaque cards -- (prim, bu, bv) are the
oracle's own triangle test's.  Ray cone (the SD trace): every hit of every SD ray of the 160 x 96 map traced from the
camera (depth input 0, no intervals), from tests/hits_checker.py with opaque cards for (t, prim) and ocpu_sd_ray /
ocpu_intersect for (d, bu, bv).

Exceptions to "each card shows both outcomes", each a property of the definition and not of a sampler: the identities
of `thresholds` (threshold 0, 1.5, NaN, constant alpha), the 1 x 1 texture of `shapes` (one texel whatever the
coordinate) and the ladder cards past the last mip (they read the 1 x 1 mip only)."""
import ctypes as C
import types

import numpy as np
import pytest

import alpha_checker as AC
import alpha_edge_scenes as E
import hits_checker
import mvec_checker as MV
from alpha_edge_scenes import CONE_SCENES, LOD0_SCENES, camera, oscene, sd_params

F = np.float32

# The counts each frame must reach at least (measured counts are an order of magnitude above these except for the
# carries, whose rate is one hit in 512 per axis by construction: the fraction rounds to 256 / 256 on 1 / 512 of a
# texel).  Keys: (scene, mode).
MINIMUM = {
    ("shapes", "lod0"): dict(carry_x=8, carry_y=8, tap_left=50, tap_right=50, tap_above=50, tap_below=50,
                             one_texel_x=1000, one_texel_y=1000, qf_zero=10000),
    ("uv_domain", "lod0"): dict(carry_x=8, carry_y=8, tap_left=50, tap_right=50, tap_above=50, tap_below=50),
    ("thresholds", "lod0"): dict(carry_x=4, carry_y=4, tap_left=50, tap_right=50, tap_above=50, tap_below=50),
    ("lod_ladder", "cone"): dict(carry_x=8, carry_y=8, carry_lod=3, tap_left=50, tap_right=50, tap_above=50,
                                 tap_below=50, one_texel_x=500, one_texel_y=500, lod_clamped_low=500,
                                 lod_clamped_high=500, qf_zero=500, last_mip=500, blend=5000),
    ("uv_domain", "cone"): dict(carry_x=4, carry_y=4, tap_left=50, tap_right=50, tap_above=50, tap_below=50,
                                blend=5000),
}


@pytest.fixture(scope="session")
def mv(oracle, tmp_path_factory):
    return MV.build(oracle, tmp_path_factory.mktemp("alpha_edges_mvec"))


@pytest.fixture(scope="session")
def hr(oracle, tmp_path_factory):
    return hits_checker.build(oracle, tmp_path_factory.mktemp("alpha_edges_hits"))


def lod0_tuples(oracle, mv, scene, positions=None):
    """(prim, bu, bv) of the card behind every pixel of the 192 x 128 frame that meets one, and the pixel."""
    cfg = E.frame_config()
    cam, _ = camera(oracle, cfg)
    pos = scene.positions if positions is None else positions
    r = MV.run(oracle, mv, E.opaque_variant(scene), pos, pos, cam, cam, (cfg.fb_w, cfg.fb_h), 0)
    hit = (r["prim"] != MV.MISS) & (r["prim"] >= 2)  # primitives 0 and 1: the backdrop
    ys, xs = np.nonzero(hit)
    return types.SimpleNamespace(prim=r["prim"][hit].astype(np.int64), bu=r["tuv"][hit][:, 1], bv=r["tuv"][hit][:, 2],
                                 t=r["tuv"][hit][:, 0], x=xs, y=ys, shape=(cfg.fb_h, cfg.fb_w))


def cone_tuples(oracle, hr, scene):
    """(prim, bu, bv, t, d) of every card hit of every ray of the 160 x 96 SD map, the texel, and the spread."""
    W, H = E.VISIBLE
    cfg = E.frame_config(guard=0)
    _, ocam = camera(oracle, cfg)
    osc = oracle.Scene(scene.positions, scene.indices, scene.flags)
    sdp = sd_params(oracle)
    z = np.zeros((H, W), F)
    cap = hits_checker.CAP
    cnt, t, prim = np.zeros((H, W), np.uint32), np.zeros((H, W, cap), F), np.zeros((H, W, cap), np.uint32)
    zt = np.zeros((H, W, cap), F)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    hr.hits_ref(osc.h, 0, p(osc.positions), p(osc.indices), p(osc.flags), len(osc.indices), C.byref(ocam), C.byref(sdp),
                p(z), W, H, None, None, W, H, cap, p(cnt), p(t), p(prim), p(zt), oracle.effective_cpus())
    assert cnt.max() <= cap
    tri = scene.positions[scene.indices]
    out = []
    for y in range(H):
        for x in range(W):
            if cnt[y, x] == 0:
                continue
            o, d, *_ = oracle.sd_ray(ocam, sdp, z, None, None, W, H, x, y)
            o, d = o.copy(), d.copy()
            for k in range(cnt[y, x]):
                q = int(prim[y, x, k])
                if q < 2:
                    continue
                hit, tt, bu, bv, _ = oracle.intersect(o, d, tri[q, 0], tri[q, 1], tri[q, 2])
                assert hit and F(tt) == t[y, x, k]
                out.append((q, bu, bv, tt, d[0], d[1], d[2], x, y))
    a = np.array(out, np.float64)
    return types.SimpleNamespace(prim=a[:, 0].astype(np.int64), bu=a[:, 1].astype(F), bv=a[:, 2].astype(F),
                                 t=a[:, 3].astype(F), d=a[:, 4:7].astype(F), x=a[:, 7].astype(np.int64),
                                 y=a[:, 8].astype(np.int64), shape=(H, W),
                                 spread=oracle.ray_cone_spread(E.FOCAL, H))


_frames = {}


def frame(oracle, mv, hr, name, mode):
    """The tuples of (scene, mode) with the checker's alpha, edges and decisions -- computed once."""
    if (name, mode) not in _frames:
        scene, cards = E.build(name)
        ck = AC.Checker(scene)
        if mode == "lod0":
            tp = lod0_tuples(oracle, mv, scene)
            alpha, edges, detail = ck.value(tp.prim, tp.bu, tp.bv)
        else:
            tp = cone_tuples(oracle, hr, scene)
            alpha, edges, detail = ck.value(tp.prim, tp.bu, tp.bv, tp.t, tp.d, tp.spread)
        _frames[name, mode] = types.SimpleNamespace(scene=scene, cards=cards, ck=ck, tp=tp, alpha=alpha, edges=edges,
                                                    detail=detail, kept=ck.kept(alpha, detail["mat"]))
    return _frames[name, mode]


CASES = [(n, "lod0") for n in LOD0_SCENES] + [(n, "cone") for n in CONE_SCENES]
IDS = [f"{n}-{m}" for n, m in CASES]


def _same_float(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("name,mode", CASES, ids=IDS)
def test_oracle_equals_checker_on_the_frames_hits(oracle, mv, hr, name, mode):
    """ocpu_alpha_value and ocpu_alpha_fails on every hit tuple of the frame: the checker's value bit for bit, and
    its decision."""
    f = frame(oracle, mv, hr, name, mode)
    osc, tp = oscene(oracle, f.scene), f.tp
    n = tp.prim.size
    assert n >= 2000
    got, fails = np.zeros(n, F), np.zeros(n, bool)
    for i in range(n):
        kw = {} if mode == "lod0" else dict(lod_ray_cone=True, t=float(tp.t[i]), d=tp.d[i], spread=tp.spread)
        got[i] = osc.alpha_value(int(tp.prim[i]), float(tp.bu[i]), float(tp.bv[i]), **kw)
        fails[i] = osc.alpha_fails(int(tp.prim[i]), float(tp.bu[i]), float(tp.bv[i]), **kw)
    bad = np.flatnonzero(~_same_float(got, f.alpha))
    assert bad.size == 0, (name, mode, bad.size, [(int(tp.prim[i]), float(got[i]), float(f.alpha[i])) for i in bad[:5]])
    assert np.array_equal(~fails, f.kept), (name, mode, int((~fails != f.kept).sum()))
    for m, thr in enumerate(f.ck.thresholds):
        assert _same_float(osc.alpha_threshold(m), thr), (m, thr)


@pytest.mark.parametrize("name,mode", CASES, ids=IDS)
def test_frames_reach_their_edges(oracle, mv, hr, name, mode):
    f = frame(oracle, mv, hr, name, mode)
    counts = {k: int(v.sum()) for k, v in f.edges.items()}
    print(name, mode, "hits", f.tp.prim.size, counts)
    for k, least in MINIMUM[name, mode].items():
        assert counts[k] >= least, (name, mode, k, counts[k], least)
    if mode == "lod0":  # LOD 0 means LOD 0
        assert counts["blend"] == 0 and (f.detail["l0"] <= 0).all()


def test_every_edge_is_reached_by_some_frame(oracle, mv, hr):
    reached = set()
    for name, mode in CASES:
        reached |= {k for k, v in frame(oracle, mv, hr, name, mode).edges.items() if v.any()}
    assert reached == set(AC.EDGES)


def test_ladder_reads_every_mip_and_both_clamps(oracle, mv, hr):
    f = frame(oracle, mv, hr, "lod_ladder", "cone")
    for ti, chain in enumerate(f.ck.chains):
        sel = f.detail["tex"] == ti
        first = f.detail["l0"][sel]
        second = first[f.edges["blend"][sel]] + 1
        read = set(first.tolist()) | set(second.tolist())
        if chain[0].shape == (3, 16):
            # the 16 x 3 texture is there for its mips of height 1 beside a width above 1 (8 x 1, 4 x 1, 2 x 1: the
            # max(1, h >> 1) of the device's mip-offset loop); mip 0 and the clamps are the other textures'
            assert read >= {1, 2, 3, 4} and (f.edges["one_texel_y"][sel] & ~f.edges["one_texel_x"][sel]).sum() >= 500
            continue
        assert read == set(range(len(chain))), (ti, sorted(read))
        for k in ("lod_clamped_low", "lod_clamped_high", "last_mip", "blend"):
            assert f.edges[k][sel].sum() >= 100, (ti, k)
        # the last interval with a non-zero fraction
        assert (f.edges["blend"][sel] & (first == len(chain) - 2)).sum() >= 100, ti


@pytest.mark.parametrize("name,mode", CASES, ids=IDS)
def test_cards_show_both_outcomes(oracle, mv, hr, name, mode):
    f = frame(oracle, mv, hr, name, mode)
    for c in f.cards:
        sel = np.isin(f.tp.prim, c.prims)
        assert sel.sum() >= 100, (name, c.name, "the card is hardly seen")
        k = f.kept[sel]
        if c.identity is None:
            assert k.any() and not k.all(), (name, mode, c.name, int(k.sum()), int(sel.sum()))
        elif c.identity == "kept":
            assert k.all(), (name, c.name)
        elif c.identity == "discarded":
            assert not k.any(), (name, c.name)
        else:  # "constant": one texel whatever the coordinate (its two lerps round, so the bits may differ): one outcome
            assert k.all() or not k.any(), (name, c.name)


def test_the_rendered_depth_is_the_decision(oracle, mv, hr):
    """The oracle's G-buffer of each LOD 0 frame shows the card's depth exactly where the checker keeps the hit."""
    for name in LOD0_SCENES:
        f = frame(oracle, mv, hr, name, "lod0")
        cfg = E.frame_config()
        _, ocam = camera(oracle, cfg)
        z, _ = oracle.gbuffer(oscene(oracle, f.scene), ocam, cfg.fb_w, cfg.fb_h, 0)
        zo, _ = oracle.gbuffer(oscene(oracle, E.opaque_variant(f.scene)), ocam, cfg.fb_w, cfg.fb_h, 0)
        shows_card = (z.view(np.uint32) == zo.view(np.uint32))[f.tp.y, f.tp.x]
        assert np.array_equal(shows_card, f.kept), (name, int((shows_card != f.kept).sum()))


def _sd(oracle, scene, impl=3):
    W, H = E.VISIBLE
    _, ocam = camera(oracle, E.frame_config(guard=0))
    return oracle.sd_trace(oscene(oracle, scene), ocam, sd_params(oracle, impl=impl), np.zeros((H, W), F), None, None,
                           W, H)[0]


def test_threshold_identities(oracle, mv, hr):
    """Without the oracle's sampler: threshold 0, an all-255 texture under 1.0, alpha = half(threshold), a NaN alpha
    and a NaN threshold keep every hit (`alpha < threshold` is false) -- the card is an opaque one; threshold 1.5 and an
    alpha one float32 below half(threshold) discard every hit -- there is no card.  The oracle's G-buffer and SD maps
    of the scene are those of the scene so rewritten."""
    scene, cards = E.build("thresholds")
    assert {c.identity for c in cards} == {None, "kept", "discarded"}
    variant = E.identity_variant(scene, cards)
    assert variant.indices.shape[0] == scene.indices.shape[0] - 2 * sum(c.identity == "discarded" for c in cards)
    cfg = E.frame_config()
    _, ocam = camera(oracle, cfg)
    for cull in (0, 1):
        a = oracle.gbuffer(oscene(oracle, scene), ocam, cfg.fb_w, cfg.fb_h, cull)
        b = oracle.gbuffer(oscene(oracle, variant), ocam, cfg.fb_w, cfg.fb_h, cull)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    # The Default reservoir counts a hit before its alpha test (Common.slangh:136-175, tests/test_alpha.py
    # test_default_reservoir_counts_failed_hits), so a card that discards every hit is not "no card" to it: there only
    # the "kept" half of the rewrite holds
    kept_only = E.identity_variant(scene, [c for c in cards if c.identity == "kept"])
    for impl, v in ((0, kept_only), (1, variant), (3, variant)):
        assert np.array_equal(_sd(oracle, scene, impl).view(np.uint32), _sd(oracle, v, impl).view(np.uint32)), impl
    # and the identities do something: with every card opaque, or none there, the frame differs
    z = oracle.gbuffer(oscene(oracle, scene), ocam, cfg.fb_w, cfg.fb_h, 0)[0]
    zo = oracle.gbuffer(oscene(oracle, E.opaque_variant(scene)), ocam, cfg.fb_w, cfg.fb_h, 0)[0]
    assert (z != zo).sum() > 1000 and (z == zo).sum() > 1000


def test_nan_threshold_survives_the_float16_rounding(oracle):
    """round_half of a NaN threshold: the oracle's and the checker's stay NaN, so `alpha < threshold` is false and the
    hit is kept (the host's round_half returns a NaN unchanged, csrc/rsd_host.cpp; the device identity is in
    tests/test_gpu_alpha_edges.py)."""
    scene, cards = E.build("thresholds")
    m = next(c.material for c in cards if c.name == "NaN threshold")
    assert np.isnan(scene.alpha.thresholds[m]) and np.isnan(AC.half(scene.alpha.thresholds[m]))
    assert np.isnan(oscene(oracle, scene).alpha_threshold(m))


def test_moved_scenes_keep_their_cards_in_view(oracle, mv):
    """The dynamic path's positions (alpha_edge_scenes.moved): the cards move, the backdrop does not, and every card
    still shows both outcomes where it must."""
    for name in ("shapes", "uv_domain"):
        scene, cards = E.build(name)
        ck = AC.Checker(scene)
        for step in (1, 2):
            p = E.moved(scene, step)
            assert np.array_equal(p[:4], scene.positions[:4]) and (p[4:] != scene.positions[4:]).any(axis=1).all()
            tp = lod0_tuples(oracle, mv, scene, p)
            alpha, _, detail = ck.value(tp.prim, tp.bu, tp.bv)
            kept = ck.kept(alpha, detail["mat"])
            for c in cards:
                k = kept[np.isin(tp.prim, c.prims)]
                assert k.size >= 100 and (c.identity is not None or (k.any() and not k.all())), (name, step, c.name)


def _device_mip(w, h, level, clamp=True):
    """csrc/alpha_test.h alpha_sample's mip-offset loop restated: (texel offset, width, height) of mip `level`;
    clamp=False is the mutant `w >> 1` without the max(1, .)."""
    off = 0
    for _ in range(level):
        off += w * h
        w, h = (max(1, w >> 1), max(1, h >> 1)) if clamp else (w >> 1, h >> 1)
    return off, w, h


def test_the_mip_loop_needs_its_clamp_to_one(oracle, mv, hr):
    """The device's mip-offset loop gives the checker's chain (offsets and sizes of every mip of every texture of the
    four scenes).  Without its max(1, .) a chain whose one axis reaches 1 before the other gets a mip of width or
    height 0 -- a division by zero in the texel addressing, which is why this mutant is judged here and not run on a
    device: the ladder's 16 x 3 texture has three such mips (8 x 1, 4 x 1, 2 x 1 become 8 x 0, ...), and the SD rays
    of `lod_ladder` read them on hundreds of hits, so every SD-trace test of that scene runs the mutated lines with
    other sizes than the oracle's.  The square 64 x 64 and the 5 x 7 chain (5 -> 2 -> 1, 7 -> 3 -> 1) cannot tell."""
    for name in E.NAMES:
        scene, _ = E.build(name)
        for tex, chain in zip(scene.alpha.textures, AC.Checker(scene).chains):
            h, w = tex.shape
            sizes = [c.shape for c in chain]
            for l in range(len(chain)):
                off, mw, mh = _device_mip(w, h, l)
                assert (off, mh, mw) == (sum(a * b for a, b in sizes[:l]), *sizes[l]), (name, tex.shape, l)
    f = frame(oracle, mv, hr, "lod_ladder", "cone")
    broken = np.zeros(f.tp.prim.size, bool)
    for ti, chain in enumerate(f.ck.chains):
        h, w = chain[0].shape
        differs = np.array([_device_mip(w, h, l) != _device_mip(w, h, l, clamp=False) for l in range(len(chain) + 1)])
        sel = f.detail["tex"] == ti
        l0 = f.detail["l0"][sel]
        hit = differs[l0] | (f.edges["blend"][sel] & differs[l0 + 1])
        assert hit.any() == (chain[0].shape == (3, 16)), (ti, chain[0].shape)
        broken[sel] = hit
    assert broken.sum() >= 500, int(broken.sum())
