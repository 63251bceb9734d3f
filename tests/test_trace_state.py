"""The cases and sequences of tests/test_gpu_trace_state.py (SD-trace state carried between calls: the SdWorkspace of
csrc/rsd_internal.h), as plain data, and -- on the oracle alone -- the preconditions that keep that test from passing
vacuously: every case has live rays, texels at DEFAULT_DEPTH and texels away from it, and any two cases that follow
each other in a sequence have expected maps that differ, so that a stale ray table, a stale workspace section or a
queue-control word left behind by the previous call shows as wrong bits.

A case is a whole SD-trace call: scene, frame, N, MAX_COUNT, implementation, camera and the trace's inputs (linear depth
and the two interval maps), all from the oracle, so the GPU test uploads them and depends on no other kernel."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

import scenes_adversarial as SA
from helpers import (SENTINEL, odd_frame, odd_frame_config, odd_second_pose, sentinel_array,
                     small_frame_config, to_oracle)

D, CM, KB = 0, 1, 3  # rsd_sd_implementation: Default, CoverageMask, KBuffer
DEFAULT_DEPTH = np.float32(3.40282347e+37)  # the cleared value of a map; 1 with normalisation, which SVAO's SD pass has
CLEARED_MIN, CLEARED_MAX = 0x7F7FFFFF, 0  # what rsd_svao_clear_intervals leaves: a dead ray

# frames of arcade_tiny (helpers.small_frame_config / odd_frame_config): (visible, guard, divisor)
BIG = ((320, 192), 32, 1)    # SD map 512 x 384: the size at which test_gpu_hybrid.py gets the hybrid walk
SMALL = ((160, 96), 16, 2)   # SD map 160 x 128
ODD = "odd_div3"             # helpers.ODD_FRAMES: SD map 60 x 39, neither a multiple of 8
# the ray-table cases cut the scene with farZ (TMax = farZ / cos is the one ray term the table's pixel-centre column
# and row feed: with the default far plane no hit lies near it and cam.jitterX / jitterY would not show in the map)
RT_FAR = 20.0
RT_JX, RT_JY = 0.04, -0.06   # cam.jitterX / jitterY, in units of the interior's width / height
RT_GUARD = 24                # the SD guard band of the guard-only step (the frame's own: 64 // 2 = 32), same map size
RT_SHIFT = (0.5, 0.25, -0.75)  # the camera translated, U, V and W unchanged


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    scene: str       # "arcade_tiny", or a scene of tests/scenes_adversarial.py (65 x 49, jitter off, zero depth input)
    frame: object    # BIG, SMALL, ODD; None for the adversarial scenes
    N: int
    max_count: int
    impl: int = D
    # The interval maps are pass 1's where pass 1 requested a ray (few texels of these small frames, and most of their
    # short intervals hold no hit) and elsewhere a pattern of unbounded (0, 0) and cleared texels (open_intervals), which
    # fills the map with hits.  open: the pattern alone; phase: the pattern moved (the cases whose first layer and channel
    # would otherwise repeat their neighbour's: the first samples of N = 1, 4 and 16 agree);
    # far, jitter, jx, jy, guard, pose ("second"), shift: see the RT_* constants
    mods: tuple = ()

    def mod(self, key, default=None):
        return dict(self.mods).get(key, default)


def _rt(name, **mods):
    return Case(name, "arcade_tiny", SMALL, 4, 8, D, tuple(sorted(dict(open=True, far=RT_FAR, **mods).items())))


_RT_STEPS = [("rt_base", {}), ("rt_nojitter", dict(jitter=False)), ("rt_jx", dict(jx=RT_JX)), ("rt_jy", dict(jy=RT_JY)),
             ("rt_guard", dict(guard=RT_GUARD)), ("rt_pose", dict(pose="second")), ("rt_shift", dict(shift=RT_SHIFT))]


def _rt_cases():
    """Each ray-table case adds exactly one change to the one before it."""
    out, acc = [], {}
    for name, change in _RT_STEPS:
        acc = dict(acc, **change)
        out.append(_rt(name, **acc))
    return out


CASES = {c.name: c for c in [
    Case("big", "arcade_tiny", BIG, 4, 8),
    Case("big_n16", "arcade_tiny", BIG, 16, 16, D, (("phase", 1),)),
    Case("small", "arcade_tiny", SMALL, 4, 8),
    Case("odd", "arcade_tiny", ODD, 4, 8),
    Case("small_n16", "arcade_tiny", SMALL, 16, 8, CM),
    Case("small_n1", "arcade_tiny", SMALL, 1, 8, D, (("phase", 1),)),
    # MAX_COUNT on `layers`, whose rays have 40 hits each, at N = 16: MAX_COUNT 4 and 8 end a ray before its 16 samples
    # are taken (arcade_tiny's rays have few hits behind the first surface, and at N = 4 the nearest MAX_COUNT >= 4 hits
    # decide every sample: those maps at MAX_COUNT 4, 8 and 32 are the same)
    Case("layers_mc32", "layers", None, 16, 32, KB, (("open", True),)),   # MAX_COUNT above K = 16: chunked
    Case("layers_mc4", "layers", None, 16, 4, D, (("open", True),)),
    Case("layers_mc8", "layers", None, 16, 8, D, (("open", True),)),
    Case("layers", "layers", None, 4, 8, D, (("open", True),)),
    Case("layers_n16", "layers", None, 16, 16, D, (("open", True), ("phase", 1))),
    Case("slivers", "slivers", None, 4, 8, D, (("open", True),)),
] + _rt_cases()}

# the orders of cases the GPU test runs on one workspace (each forwards and in reverse)
SEQUENCES = {
    "sizes": ["big", "small", "odd", "big", "small"],   # grow once, then a larger allocation with moved sections
    "samples": ["small_n16", "small_n1", "small"],      # N 16 -> 1 -> 4
    "max_count": ["layers_mc32", "layers_mc4", "layers_mc8"],  # MAX_COUNT 32 -> 4 -> 8
    "ray_table": [n for n, _ in _RT_STEPS] + ["rt_shift"],  # last: nothing changes (the cached table)
    "walks_arcade": ["big", "big_n16", "big"],          # the walk sequence's HYBRID16 step runs the N = 16 case
    "walks_layers": ["layers", "layers_n16", "layers"],
    "clean_tiles": ["big", "small"],
    "streams": ["big", "small"],
}
RT_PAIRS = {"jitter": ("rt_base", "rt_nojitter"), "jitterX": ("rt_nojitter", "rt_jx"), "jitterY": ("rt_jx", "rt_jy"),
            "guard": ("rt_jy", "rt_guard"), "pose": ("rt_guard", "rt_pose"), "pose_same_W": ("rt_pose", "rt_shift")}


def open_intervals(w, h, phase=0):
    """(rayMin, rayMax): unbounded rays in a pattern finer than a tile, cleared (dead) texels between them and in a
    block of whole tiles, which a trace leaves at DEFAULT_DEPTH.  phase: 0, 1 or 2 moves the pattern."""
    y, x = np.mgrid[0:h, 0:w]
    live = ((x // 5 + y // 3 + phase) % 3 != 0) & ~((x >= (2 * w) // 3) & (y < h // 2))
    return np.where(live, 0, CLEARED_MIN).astype(np.uint32), np.full((h, w), CLEARED_MAX, np.uint32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Built:
    """A case made concrete: the configuration, the camera and parameter structs of librsd, the inputs of the trace and
    the oracle's map.  Nothing here is written after construction."""

    def __init__(self, oracle, case, oscene, scene):
        from rsd.frame import look_at, make_camera, make_vao, sd_params
        self.case, self.scene, self.osc = case, scene, oscene
        if case.frame is None:
            cfg = SA.frame_config(N=case.N, max_count=case.max_count, impl=case.impl)
        elif case.frame == ODD:
            cfg = odd_frame_config(odd_frame(ODD), N=case.N, max_count=case.max_count, implementation=case.impl)
        else:
            visible, guard, divisor = case.frame
            cfg = small_frame_config(visible=visible, guard=guard, divisor=divisor, N=case.N,
                                     max_count=case.max_count, impl=case.impl)
        self.cfg = cfg = dataclasses.replace(cfg, numerics="exact", jitter=bool(case.mod("jitter", cfg.jitter)))
        if case.mod("pose") == "second":
            pos, target, up = odd_second_pose(scene)
        else:
            pos, target, up = (scene.camera[k] for k in ("pos", "target", "up"))
        cam = look_at(pos, target, up, cfg) if case.mod("pose") else make_camera(scene, cfg)
        if case.mod("shift"):
            for k, d in enumerate(case.mod("shift")):
                cam.posW[k] = float(np.float32(cam.posW[k]) + np.float32(d))
        if case.mod("jx") is not None:
            cam.jitterX = case.mod("jx")
        if case.mod("jy") is not None:
            cam.jitterY = case.mod("jy")
        if case.mod("far") is not None:
            cam.farZ = case.mod("far")
        self.cam, self.ocam = cam, to_oracle(cam, oracle.Camera)
        self.vao, self.sd_w, self.sd_h = make_vao(cfg)
        self.sdp = sd_params(cfg, self.vao.sdGuard)
        if case.mod("guard") is not None:
            self.sdp.guard_band = case.mod("guard")
        self.osdp = to_oracle(self.sdp, oracle.SDParams)
        self.default = np.float32(1.0) if self.sdp.normalize else DEFAULT_DEPTH
        w, h = self.sd_w, self.sd_h
        if case.frame is None:
            self.depth = np.zeros((cfg.fb_h, cfg.fb_w), np.float32)
        else:
            self.depth, normals = oracle.gbuffer(oscene, self.ocam, cfg.fb_w, cfg.fb_h, cfg.cull_mode)
        self.rmin, self.rmax = open_intervals(w, h, case.mod("phase", 0))
        if not case.mod("open"):
            from rsd.frame import svao_params
            svp = to_oracle(svao_params(cfg), oracle.SVAOParams)
            _, _, rmin, rmax = oracle.svao_pass1(self.ocam, to_oracle(self.vao, oracle.VAOData), svp, self.depth,
                                                 normals, w, h)
            self.touched = rmin != CLEARED_MIN
            assert self.touched.sum() > 500
            self.rmin, self.rmax = np.where(self.touched, rmin, self.rmin), np.where(self.touched, rmax, self.rmax)
        self.want, self.stats = oracle.sd_trace(oscene, self.ocam, self.osdp, self.depth, self.rmin, self.rmax, w, h)
        for a in (self.depth, self.rmin, self.rmax, self.want):
            a.setflags(write=False)

    def want_cleared(self, oracle):
        """The oracle's map over cleared intervals: no live ray."""
        rmin = np.full((self.sd_h, self.sd_w), CLEARED_MIN, np.uint32)
        rmax = np.full((self.sd_h, self.sd_w), CLEARED_MAX, np.uint32)
        sd, stats = oracle.sd_trace(self.osc, self.ocam, self.osdp, self.depth, rmin, rmax, self.sd_w, self.sd_h)
        assert stats[0] == 0
        return sd


_scenes, _built = {}, {}


def host_scene(name):
    from rsd.scenes import make_scene
    if name not in _scenes:
        _scenes[name] = make_scene(name) if name == "arcade_tiny" else SA.make(name)
    return _scenes[name]


def built(oracle, name) -> Built:
    """The case `name`, computed once per process and shared by every test."""
    if name not in _built:
        case = CASES[name]
        scene = host_scene(case.scene)
        key = ("oscene", case.scene)
        if key not in _scenes:
            _scenes[key] = oracle.Scene(scene.positions, scene.indices, scene.flags, scene.alpha)
        _built[name] = Built(oracle, case, _scenes[key], scene)
    return _built[name]


def differing(a, b):
    """(shapes equal, fraction of the texels of the common top-left region -- common layers and channels -- of two SD
    maps [layer][y][x][channel] whose bits differ)."""
    common = tuple(slice(0, min(p, q)) for p, q in zip(a.shape, b.shape))
    return a.shape == b.shape, float((bits(a[common]) != bits(b[common])).any(axis=(0, 3)).mean())


def neighbours():
    """Every ordered pair of different cases that follow each other in a sequence."""
    out = []
    for seq in SEQUENCES.values():
        for p, q in zip(seq, seq[1:]):
            if p != q and (p, q) not in out and (q, p) not in out:
                out.append((p, q))
    return out


def assert_distinct(oracle, p, q):
    """The condition on the inputs: where the shapes match the maps differ bitwise, otherwise at least 1 % of the
    common region's texels differ."""
    same_shape, frac = differing(built(oracle, p).want, built(oracle, q).want)
    print(f"{p} -> {q}: {'same shape' if same_shape else 'common region'}, {100 * frac:.2f} % of the texels differ")
    assert frac > 0.0 if same_shape else frac >= 0.01, (p, q, frac)


# ---- the preconditions

def test_the_table_names_what_the_sequences_use():
    used = {n for seq in SEQUENCES.values() for n in seq} | {"slivers"}
    assert used == set(CASES)
    assert {CASES[n].N for n in SEQUENCES["samples"]} == {1, 4, 16}
    assert [CASES[n].max_count for n in SEQUENCES["max_count"]] == [32, 4, 8]
    assert {c.impl for c in CASES.values()} == {D, CM, KB}


@pytest.mark.parametrize("name", list(CASES))
def test_case_can_show_a_fault(oracle, name):
    b = built(oracle, name)
    f = odd_frame(ODD)
    if b.case.frame == ODD:
        assert b.sd_w % 8 and b.sd_h % 8, (f.name, b.sd_w, b.sd_h)
    if b.case.frame == BIG:
        assert (b.sd_w, b.sd_h) == (512, 384)
    if b.case.frame is None:
        assert (b.sd_w, b.sd_h) == (SA.W, SA.H)
    assert b.want.shape == ((b.case.N + 3) // 4, b.sd_h, b.sd_w, min(b.case.N, 4))
    assert int(b.stats[0]) > 0, "no live ray"
    default = bits(b.want) == bits(b.default)
    print(f"{name}: {b.sd_w} x {b.sd_h}, {int(b.stats[0])} live rays, {100 * default.mean():.1f} % of the values at "
          "DEFAULT_DEPTH")
    assert default.all(axis=(0, 3)).any(), "no texel at DEFAULT_DEPTH"
    assert (~default).any(axis=(0, 3)).mean() > 0.05, "hardly a texel away from DEFAULT_DEPTH"
    # the sentinel the GPU test pre-fills the map with is no result
    sentinel = sentinel_array(b.want.shape, np.float32)
    assert (sentinel.view(np.uint8) == SENTINEL).all() and not (bits(b.want) == bits(sentinel)).any()
    # whole 8x8 tiles without a live ray (clean tiles) beside tiles with some
    live = b.rmin != CLEARED_MIN
    th, tw = b.sd_h // 8, b.sd_w // 8
    tiles = live[:th * 8, :tw * 8].reshape(th, 8, tw, 8).any(axis=(1, 3))
    assert tiles.any() and not tiles.all()
    # the cleared map differs from the case's own: a trace over cleared intervals before it must show
    assert not np.array_equal(bits(b.want_cleared(oracle)), bits(b.want))


@pytest.mark.parametrize("pair", neighbours(), ids=lambda p: "-".join(p))
def test_neighbours_in_a_sequence_differ(oracle, pair):
    assert_distinct(oracle, *pair)


@pytest.mark.parametrize("what", list(RT_PAIRS))
def test_ray_table_steps_change_one_thing_and_the_map(oracle, what):
    p, q = (built(oracle, n) for n in RT_PAIRS[what])
    assert (p.sd_w, p.sd_h) == (q.sd_w, q.sd_h)
    key = lambda b: dict(jitter=b.sdp.jitter, jitterX=b.cam.jitterX, jitterY=b.cam.jitterY, guard=b.sdp.guard_band,  # noqa: E731
                         W=tuple(b.cam.W), pos=tuple(b.cam.posW))
    changed = {k for k in key(p) if key(p)[k] != key(q)[k]}
    # (a new pose moves the camera and turns it; the translation keeps U, V and W)
    assert changed == {"pose": {"W", "pos"}, "pose_same_W": {"pos"}}.get(what, {what}), changed
    if what == "pose_same_W":
        assert all(tuple(getattr(p.cam, k)) == tuple(getattr(q.cam, k)) for k in "UVW")
    same_shape, frac = differing(p.want, q.want)
    print(f"{what}: {100 * frac:.2f} % of the texels differ")
    # more than a stray texel: a table kept from the step before must be seen
    assert same_shape and frac >= 0.01, (what, frac)


def test_identical_neighbours_would_be_noticed(oracle, monkeypatch):
    """The check of the neighbours fails when a case is the copy of the one before it."""
    monkeypatch.setitem(_built, "copy_of_big", built(oracle, "big"))
    with pytest.raises(AssertionError):
        assert_distinct(oracle, "big", "copy_of_big")
