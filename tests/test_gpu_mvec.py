"""GPU: the motion vectors of moving geometry (rsd_scene_track_motion, rsd_scene_motion_begin_frame,
rsd_gbuffer_motion) against the brute-force checker of tests/native/mvec_ref.c, bit for bit.

Frames are 75 x 45 (partial 8 x 8 tiles on both axes) and 13 x 7 (smaller than one image block); scenes are
arcade_tiny and foliage_small at ~3000 triangles, the turnstile fixture and a hand-made patch.  Every output is
allocated with canaries on both sides.  Depth, normal and posW are compared with rsd_gbuffer_world's bytes on the same
scene."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest

import mvec_checker as MV
import skinning_checker
from conftest import ROOT
from helpers import assert_canaries_intact, canary

pytestmark = pytest.mark.gpu

BIG, TINY = MV.SIZES


@pytest.fixture(scope="module")
def gpu(oracle, tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rsd import abi
    from rsd.frame import Device
    d = Device(0)
    g = types.SimpleNamespace(torch=torch, abi=abi, L=abi.lib(), dev=d, O=oracle,
                              lib=MV.build(oracle, tmp_path_factory.mktemp("mvec_ref")),
                              scenes={k: MV.make_scene(k) for k in MV.SCENES})
    yield g
    torch.cuda.synchronize()
    d.close()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _motion(gpu, gs, cam, prev, size, cull, pos_w=True, mvec_w=True):
    """rsd_gbuffer_motion into canaried buffers; returns the host copies."""
    t, (W, H) = gpu.torch, size
    out = {"depth": canary(t, (H, W), t.float32), "normal": canary(t, (H, W, 4), t.float32),
           "mvec": canary(t, (H, W, 2), t.float32)}
    if pos_w:
        out["posW"] = canary(t, (H, W, 4), t.float32)
    if mvec_w:
        out["mvecW"] = canary(t, (H, W, 4), t.float32)
    gpu.abi.check(gpu.L.rsd_gbuffer_motion(gs.h, C.byref(cam), C.byref(prev), W, H, cull, _p(out["depth"].view),
                                           _p(out["normal"].view), _p(out["posW"].view) if pos_w else None,
                                           _p(out["mvec"].view), _p(out["mvecW"].view) if mvec_w else None, None),
                  "rsd_gbuffer_motion")
    assert_canaries_intact(t, out, f"rsd_gbuffer_motion {size}")
    return {k: o.numpy() for k, o in out.items()}


def _world(gpu, gs, cam, size, cull):
    t, (W, H) = gpu.torch, size
    out = {"depth": canary(t, (H, W), t.float32), "normal": canary(t, (H, W, 4), t.float32),
           "posW": canary(t, (H, W, 4), t.float32)}
    gpu.abi.check(gpu.L.rsd_gbuffer_world(gs.h, C.byref(cam), W, H, cull, _p(out["depth"].view),
                                          _p(out["normal"].view), _p(out["posW"].view), None), "rsd_gbuffer_world")
    assert_canaries_intact(t, out, f"rsd_gbuffer_world {size}")
    return {k: o.numpy() for k, o in out.items()}


def _same(got, want, what):
    bad = np.argwhere(MV.bits(got) != MV.bits(want))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _check(gpu, gs, scene, pos, prev_pos, cam, prev, size, cull, what, **kw):
    """One rsd_gbuffer_motion call against the checker(prev_pos -> pos) and rsd_gbuffer_world; returns both."""
    got = _motion(gpu, gs, cam, prev, size, cull, **kw)
    want = MV.run(gpu.O, gpu.lib, scene, pos, prev_pos, cam, prev, size, cull)
    _same(got["mvec"], want["mvec"], f"{what}: mvec")
    if "mvecW" in got:
        _same(got["mvecW"], want["mvec_w"], f"{what}: mvecW")
    world = _world(gpu, gs, cam, size, cull)
    for k in ("depth", "normal", "posW"):
        if k in got:
            assert got[k].tobytes() == world[k].tobytes(), f"{what}: {k} is not rsd_gbuffer_world's"
    assert np.array_equal(want["prim"] != MV.MISS, world["depth"] < 1.0), what
    return got, want


def _tracked(gpu, scene):
    from rsd.frame import GpuScene
    gs = GpuScene(gpu.dev, scene, dynamic=True, motion=True)
    info = gs.motion_info()
    assert info.tracked == 1 and info.snapshots == 0 and info.motion_bytes >= 12 * scene.positions.shape[0]
    return gs


def _moved_cam(scene, size):
    c = scene.camera
    return MV.camera(scene, size, pos=[c["pos"][0] + 0.3, c["pos"][1] + 0.1, c["pos"][2] - 0.2])


# ---------------------------------------------------------------------------------- 5. parity

@pytest.mark.parametrize("kind,size,cull,camera_moves", [
    ("opaque", BIG, 0, False), ("opaque", BIG, 1, False), ("opaque", BIG, 2, False), ("opaque", BIG, 1, True),
    ("alpha", BIG, 0, False), ("alpha", BIG, 1, True), ("alpha", BIG, 2, False),
    ("opaque", TINY, 1, True), ("alpha", TINY, 0, False)],
    ids=lambda v: v if isinstance(v, str) else ("x".join(map(str, v)) if isinstance(v, tuple) else str(v)))
def test_parity(gpu, kind, size, cull, camera_moves):
    """upload dynamic, track_motion, begin_frame, update_positions(P1), rsd_gbuffer_motion: mvec and mvecW are the
    checker's (P0 -> P1) bits, divisions included; depth, normal and posW are rsd_gbuffer_world's bytes; with the
    optional outputs left out mvec keeps its bits.  On foliage_small the alpha test decides the winning triangle: a
    pixel seen through a cut-out takes the motion of the surface behind it (the checker without the alpha data
    differs there, and the kernel agrees with the one with it)."""
    scene = gpu.scenes[kind]
    p0, p1 = scene.positions, MV.moved(scene, 1)
    prev = MV.camera(scene, size)
    cam = _moved_cam(scene, size) if camera_moves else prev
    gs = _tracked(gpu, scene)
    try:
        gs.begin_frame()
        gs.update_positions(p1)
        what = f"{kind} {size} cull {cull} camera {camera_moves}"
        got, want = _check(gpu, gs, scene, p1, p0, cam, prev, size, cull, what)
        hit = want["prim"] != MV.MISS
        assert hit.any() and MV.bits(got["mvecW"])[hit].any() and not MV.bits(got["mvecW"])[~hit].any()
        assert not MV.bits(got["mvec"])[~hit].any(), "a miss is (0, 0)"
        bare = _motion(gpu, gs, cam, prev, size, cull, pos_w=False, mvec_w=False)
        assert bare["mvec"].tobytes() == got["mvec"].tobytes() and bare["depth"].tobytes() == got["depth"].tobytes()
        if kind == "alpha" and size == BIG:
            opaque = dataclasses.replace(scene, alpha=None)
            front = MV.run(gpu.O, gpu.lib, opaque, p1, p0, cam, prev, size, cull)
            through = hit & (front["prim"] != want["prim"])
            assert through.any(), "no pixel looks through a cut-out: the case does not test the alpha path"
            assert (MV.bits(front["mvec_w"])[through] != MV.bits(got["mvecW"])[through]).any()
    finally:
        gpu.torch.cuda.synchronize()
        gs.release()


# ---------------------------------------------------------------------------------- 6. the snapshot rule

def test_snapshot_rule(gpu):
    """Updates never snapshot: P0 -> P1 -> P2 without begin_frame measures P0 -> P2; begin_frame, then P2 -> P3
    measures P2 -> P3; begin_frame twice without an update counts one snapshot; and after begin_frame with no
    update every pixel's mvecW is +0 bits."""
    scene, size, cull = gpu.scenes["opaque"], BIG, 1
    p0, p1, p2, p3 = scene.positions, MV.moved(scene, 1), MV.moved(scene, 2, part=(-0.2, 0.1, 0.3)), MV.moved(scene, 3)
    cam = MV.camera(scene, size)
    gs = _tracked(gpu, scene)
    try:
        gs.begin_frame()  # nothing moved since track_motion: enqueues nothing
        assert gs.motion_info().snapshots == 0
        gs.update_positions(p1)
        gs.update_positions(p2)
        _check(gpu, gs, scene, p2, p0, cam, cam, size, cull, "P0 -> P1 -> P2")
        gs.begin_frame()
        assert gs.motion_info().snapshots == 1
        gs.update_positions(p3)
        _check(gpu, gs, scene, p3, p2, cam, cam, size, cull, "begin_frame, P2 -> P3")
        gs.begin_frame()
        gs.begin_frame()
        assert gs.motion_info().snapshots == 2, "the second begin_frame without an update enqueues nothing"
        got, _ = _check(gpu, gs, scene, p3, p3, cam, cam, size, cull, "begin_frame, no update")
        assert not MV.bits(got["mvecW"]).any(), "nothing moved: mvecW is +0 on every pixel"
        assert gs.dynamic_info().updates == 3
    finally:
        gpu.torch.cuda.synchronize()
        gs.release()


# ---------------------------------------------------------------------------------- 7. the other update paths

def test_update_subset(gpu):
    """update_subset moves 1 % of the vertices: pixels whose winning triangle has no moved vertex have mvecW == +0
    bits, and everything equals the checker."""
    scene, size, cull = gpu.scenes["opaque"], BIG, 0
    nv = scene.positions.shape[0]
    ids = np.random.default_rng(7).choice(nv, max(1, nv // 100), replace=False).astype(np.uint32)
    p1 = scene.positions.copy()
    p1[ids] += np.float32((0.25, 0.5, -0.25))
    cam = MV.camera(scene, size)
    gs = _tracked(gpu, scene)
    try:
        gs.update_subset(ids, p1[ids])
        got, want = _check(gpu, gs, scene, p1, scene.positions, cam, cam, size, cull, "update_subset")
        hit = want["prim"] != MV.MISS
        is_moved = np.zeros(nv, bool)
        is_moved[ids] = True
        touched = np.zeros(hit.shape, bool)
        touched[hit] = is_moved[scene.indices[want["prim"][hit]]].any(axis=-1)
        assert touched.any() and (hit & ~touched).any()
        assert not MV.bits(got["mvecW"])[~touched].any(), "an untouched triangle's pixel has mvecW == +0"
        assert MV.bits(got["mvecW"])[touched].any()
    finally:
        gpu.torch.cuda.synchronize()
        gs.release()


def test_update_pose(gpu):
    """update_pose on the turnstile rig at t = 0.25, begin_frame, then t = 0.5: the checker fed by
    tests/skinning_checker.py's positions of the two poses."""
    from rsd.pyscene import load_pyscene
    scene = load_pyscene(ROOT / "tests" / "fixtures" / "turnstile.pyscene").build("turnstile")
    size, cull = BIG, 1
    pose = lambda t: skinning_checker.posed(scene.positions, scene.rig, scene.rig.matrices(t))
    a, b = pose(0.25), pose(0.5)
    assert MV.bits(a).tobytes() != MV.bits(b).tobytes()
    cam = MV.camera(scene, size)
    gs = _tracked(gpu, scene)
    try:
        gs.animate(0.25)
        gs.begin_frame()
        gs.animate(0.5)
        got, want = _check(gpu, gs, scene, b, a, cam, cam, size, cull, "update_pose")
        assert MV.bits(got["mvecW"]).any(), "the rotor moved"
        assert gs.motion_info().snapshots == 1
    finally:
        gpu.torch.cuda.synchronize()
        gs.release()


# ---------------------------------------------------------------------------------- 8. behind the previous camera

def test_behind_the_previous_camera(gpu):
    """A patch of triangles whose P0 lies behind the camera plane and whose P1 is in view: its pixels read (2, 2),
    as the checker says; the static wall behind it reads the camera-only vectors (0 here)."""
    from rsd.scenes import Scene

    def quad(x0, x1, y0, y1, z):
        return [[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]]

    p1 = np.array(quad(-4, 4, -3, 3, -2.0) + quad(-0.5, 0.25, -0.4, 0.3, 0.0), np.float32)
    p0 = p1.copy()
    p0[4:, 2] = 5.0  # behind the camera at z = 3 looking down -z
    idx = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.uint32)
    scene = Scene("patch", p0, idx, np.ones(4, np.uint32),  # double-sided
                  dict(pos=[0.0, 0.0, 3.0], target=[0.0, 0.0, 0.0], up=[0.0, 1.0, 0.0]))
    for size in (BIG, TINY):
        cam = MV.camera(scene, size)
        gs = _tracked(gpu, scene)
        try:
            gs.update_positions(p1)
            got, want = _check(gpu, gs, scene, p1, p0, cam, cam, size, 1, f"behind {size}")
            patch = want["prim"] >= 2
            patch &= want["prim"] != MV.MISS
            wall = want["prim"] < 2
            assert patch.any() and wall.any()
            assert (got["mvec"][patch] == 2.0).all(), "previous position behind the previous camera: (2, 2)"
            assert not MV.bits(got["mvec"][wall]).any() or np.abs(got["mvec"][wall]).max() < 1e-6
            assert np.abs(got["mvecW"][patch][:, 2] - 5.0).max() < 1e-5  # three rounded products and two sums
        finally:
            gpu.torch.cuda.synchronize()
            gs.release()


# ---------------------------------------------------------------------------------- 9. refusals

def test_refusals_and_byte_counts(gpu):
    """rsd_gbuffer_motion on an untracked dynamic scene and rsd_scene_track_motion on a static scene are
    RSD_ERR_INVALID_ARG with their messages; tracking leaves dynamic_bytes alone and adds motion_bytes to the
    scene's device bytes, nothing else; track_motion twice is one allocation."""
    from rsd.frame import GpuScene
    scene, size = gpu.scenes["opaque"], TINY
    W, H = size
    cam = MV.camera(scene, size)
    t, L, abi = gpu.torch, gpu.L, gpu.abi
    plain, tracked, static = (GpuScene(gpu.dev, scene, dynamic=True), GpuScene(gpu.dev, scene, dynamic=True),
                              GpuScene(gpu.dev, scene))
    try:
        out = {k: canary(t, (H, W, n), t.float32) for k, n in (("depth", 1), ("normal", 4), ("mvec", 2))}
        st = L.rsd_gbuffer_motion(plain.h, C.byref(cam), C.byref(cam), W, H, 1, _p(out["depth"].view),
                                  _p(out["normal"].view), None, _p(out["mvec"].view), None, None)
        assert st == abi.ERR_INVALID_ARG and b"motion is not tracked" in L.rsd_last_error()
        assert_canaries_intact(t, out, "a refused rsd_gbuffer_motion")
        assert all(o.untouched() for o in out.values())
        assert L.rsd_scene_motion_begin_frame(plain.h, None) == abi.ERR_INVALID_ARG
        assert b"motion is not tracked" in L.rsd_last_error()
        assert L.rsd_scene_track_motion(static.h) == abi.ERR_INVALID_ARG
        assert b"rsd_scene_track_motion" in L.rsd_last_error() and b"not dynamic" in L.rsd_last_error()
        assert L.rsd_scene_motion_begin_frame(static.h, None) == abi.ERR_INVALID_ARG
        assert plain.motion_info().tracked == 0 and plain.motion_info().motion_bytes == 0
        assert static.motion_info().tracked == 0

        def device_bytes(gs):
            info = abi.SceneInfo()
            abi.check(L.rsd_scene_info_get(gs.h, C.byref(info)), "rsd_scene_info_get")
            return info.device_bytes

        before = (tracked.dynamic_info().dynamic_bytes, device_bytes(tracked))
        assert before == (plain.dynamic_info().dynamic_bytes, device_bytes(plain))
        tracked.track_motion()
        tracked.track_motion()
        m = tracked.motion_info()
        assert m.tracked == 1 and m.snapshots == 0 and m.motion_bytes == 12 * scene.positions.shape[0]
        assert tracked.dynamic_info().dynamic_bytes == before[0] == plain.dynamic_info().dynamic_bytes
        assert device_bytes(tracked) - device_bytes(plain) == m.motion_bytes
    finally:
        t.cuda.synchronize()
        for s in (plain, tracked, static):
            s.release()


def test_python_entries(gpu):
    """Renderer.gbuffer_motion and rsd.temporal.motion_vectors_scene return the tensors of the same call."""
    from rsd.frame import FrameConfig, Renderer
    from rsd.temporal import motion_vectors_scene
    scene, (W, H) = gpu.scenes["opaque"], BIG
    r = Renderer(scene, FrameConfig(visible_w=W, visible_h=H, guard_band=0), dev=gpu.dev, dynamic=True, motion=True)
    try:
        prev = MV.camera(scene, BIG)
        assert bytes(prev) == bytes(r.cam)
        r.set_pose([a + b for a, b in zip(scene.camera["pos"], (0.3, 0.1, -0.2))], scene.camera["target"],
                   scene.camera["up"])
        p1 = MV.moved(scene, 1)
        r.update_positions(p1)
        a = r.gbuffer_motion(prev)
        b = motion_vectors_scene(r.gscene, r.cam, prev, W, H, cull_mode=r.cfg.cull_mode, pos_w=True)
        want = MV.run(gpu.O, gpu.lib, scene, p1, scene.positions, r.cam, prev, BIG, r.cfg.cull_mode)
        for k, w in (("mvec", "mvec"), ("mvec_w", "mvec_w")):
            _same(a[k].cpu().numpy(), want[w], f"Renderer.gbuffer_motion {k}")
            _same(b[k].cpu().numpy(), want[w], f"motion_vectors_scene {k}")
        for k in ("depth", "normal_w", "pos_w"):
            assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes()
        r.gscene.begin_frame(stream=r.stream)
        assert r.gscene.motion_info().snapshots == 1
    finally:
        r.close()
