"""GPU: animated scenes (rsd_scene_attach_rig, rsd_scene_update_pose; csrc/skinning.hip).

All comparisons are bitwise.  The pose arithmetic is stated independently in tests/skinning_checker.py; what a pose
leaves on the device is rsd_bvh_refit of the upload's tree at the checker's positions (the refit itself is pinned by
tests/test_bvh_refit.py), and what is rendered from it equals a fresh static upload of those positions and the CPU
oracle.  Frames are 75 x 45, exact numerics.  Every id handed to the device is valid: the refusals are host checks.  The last three tests
leave the inputs of order 1: denormal results, overflow, a NaN weight and an infinite rest coordinate."""
import dataclasses
import os

import numpy as np
import pytest

import morph_checker
import skinning_checker
from helpers import oracle_frame, to_oracle

pytestmark = pytest.mark.gpu

W, H = 75, 45
BLOCK = 256  # csrc/skinning.hip kPoseBlock
NM = 5       # matrices of the byte tests


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cfg(**kw):
    from rsd.frame import FrameConfig
    base = dict(visible_w=W - 16, visible_h=H - 16, guard_band=8, divisor=1, sd_guard_px=16, radius=2.0,
                numerics="exact")
    base.update(kw)
    cfg = FrameConfig(**base)
    assert (cfg.fb_w, cfg.fb_h) == (W, H)
    return cfg


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rsd.frame import Device
    d = Device(0)
    yield d
    d.close()


def _shape_scene(name):
    from rsd.ingest import load_obj
    from rsd.scenes import Scene, make_scene
    from conftest import ROOT
    cam = dict(pos=[0.0, 0.0, 3.0], target=[0.0, 0.0, 0.0], up=[0.0, 1.0, 0.0])
    if name == "one_triangle":
        return Scene(name, np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], np.float32), np.array([[0, 1, 2]], np.uint32),
                     np.zeros(1, np.uint32), cam)
    if name == "grid_24":  # x = 0 along one edge: stored as -0 there, so that an identity pose has a sign to lose
        p = np.array([[x, y, 0.25 * x * y] for y in range(4) for x in range(5)], np.float32)
        p[p == 0] = np.float32(-0.0)
        i = np.arange(20).reshape(4, 5)
        a, b, c, d = i[:-1, :-1], i[:-1, 1:], i[1:, 1:], i[1:, :-1]
        t = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 2).reshape(-1, 3).astype(np.uint32)
        return Scene(name, p, np.ascontiguousarray(t), np.zeros(24, np.uint32), cam)
    if name == "crate":
        return load_obj(ROOT / "tests" / "fixtures" / "crate.obj").build("crate")
    if name == "arcade_3000":
        return make_scene("arcade_tiny", target_tris=3000)
    raise KeyError(name)


def _rig(nv, count, order, seed, matrix_count=NM):
    """`count` distinct vertices in scattered (a random draw) or descending order; the influences cycle through rigid,
    two and four non-zero weights that do not sum to 1, and a weight-0 slot that names another matrix."""
    from rsd.animation import Rig
    rng = np.random.default_rng(seed)
    ids = rng.choice(nv, count, replace=False).astype(np.uint32)
    if order == "descending":
        ids = np.sort(ids)[::-1].copy()
    m = rng.integers(0, matrix_count, (count, 4)).astype(np.uint32)
    w = np.zeros((count, 4), np.float32)
    for i in range(count):
        kind = i % 4
        if kind == 0:
            m[i, 1:], w[i] = 0, (1, 0, 0, 0)
        elif kind == 1:
            w[i] = (0.75, 0, 0.5, 0)
        elif kind == 2:
            w[i] = (0.3, 0.2, 0.1, 0.3)
        else:
            m[i, 1] = (m[i, 0] + 1) % matrix_count  # a different matrix, weight 0: still evaluated
            w[i] = (0.6, 0, 0, 0.3)
    return Rig(ids, m, w, matrix_count)


def _poses(seed):
    rng = np.random.default_rng(seed)
    A = skinning_checker.random_matrices(rng, NM)
    A[NM - 1, [3, 7, 11]] = (500.0, -20.0, 3.0)  # one matrix carries its vertices far away
    B = skinning_checker.random_matrices(rng, NM, translation=3.0)
    return A, B, skinning_checker.identity_matrices(NM)


CASES = [("one_triangle", 0, "scattered"), ("one_triangle", 1, "scattered"), ("one_triangle", 3, "descending"),
         ("grid_24", 3, "scattered"), ("grid_24", "all", "descending"), ("crate", "all", "scattered"),
         ("arcade_3000", 63, "scattered"), ("arcade_3000", 64, "descending"), ("arcade_3000", 65, "scattered"),
         ("arcade_3000", BLOCK - 1, "descending"), ("arcade_3000", BLOCK, "scattered"),
         ("arcade_3000", BLOCK + 1, "scattered"), ("arcade_3000", "all", "scattered"),
         ("arcade_3000", "all", "descending")]


@pytest.mark.parametrize("name,count,order", CASES, ids=[f"{n}-{c}-{o}" for n, c, o in CASES])
def test_poses_leave_the_host_refit_of_the_checkers_positions(gpu, name, count, order):
    """A (host table) -> B (device table) -> identity -> A on one scene object."""
    import torch
    from rsd.frame import GpuScene, host_bvh, host_bvh_refit
    scene = _shape_scene(name)
    nv = scene.positions.shape[0]
    n = nv if count == "all" else count
    assert n <= nv and (count == "all" or name != "arcade_3000" or nv > BLOCK + 1)
    rig = _rig(nv, n, order, seed=7 + n)
    A, B, I = _poses(11)
    built, off = host_bvh(scene)
    gs = GpuScene(gpu, scene, dynamic=True)
    try:
        gs.attach_rig(rig)
        info = gs.rig_info()
        assert (info.attached, info.count, info.matrix_count) == (1, n, NM) and info.rig_bytes > 0
        steps = [("A host", A, A), ("B device", B, torch.from_numpy(B).cuda()), ("identity", I, I), ("A again", A, A)]
        for k, (what, M, arg) in enumerate(steps):
            gs.update_pose(arg)
            p = skinning_checker.posed(scene.positions, rig, M)
            want = host_bvh_refit(built, off, scene.indices, p)
            have, _ = gs.export_bvh()
            bad = np.flatnonzero(_u32(have) != _u32(want))
            assert bad.size == 0, (name, n, what, bad.size, bad[:8])
            if what == "identity" and name == "grid_24" and n == nv:
                zero = _u32(scene.positions) == 0x80000000
                assert zero.any() and (_u32(p)[zero] == 0).all(), "-0 + +0 = +0: the identity pose is not the upload"
                assert not np.array_equal(_u32(have), _u32(built))
            assert gs.dynamic_info().updates == k + 1
        assert gs.dynamic_info().entry_grid_current == (0 if gs.info.entry_cells else 1)
    finally:
        gs.release()


def test_vertices_outside_the_rig_keep_their_upload_bytes(gpu):
    from rsd.frame import GpuScene
    scene = _shape_scene("arcade_3000")
    nv = scene.positions.shape[0]
    rig = _rig(nv, nv // 5, "scattered", seed=3)
    A, B, _ = _poses(5)
    gs = GpuScene(gpu, scene, dynamic=True)
    try:
        before, off = gs.export_bvh()
        gs.attach_rig(rig)
        still = ~np.isin(scene.indices, rig.vertex_ids).any(axis=1)
        assert 100 < still.sum() < scene.indices.shape[0] - 100
        for M in (A, B):
            gs.update_pose(M)
            after, _ = gs.export_bvh()
            r0 = _u32(before)[4 * off:].reshape(-1)[:12 * scene.indices.shape[0]].reshape(-1, 12)
            r1 = _u32(after)[4 * off:].reshape(-1)[:12 * scene.indices.shape[0]].reshape(-1, 12)
            assert np.array_equal(r0[:, 3], r1[:, 3]), "primitive ids stay"
            keep = still[r0[:, 3]]
            assert np.array_equal(r0[keep], r1[keep]) and not np.array_equal(r0[~keep], r1[~keep])
    finally:
        gs.release()


def test_pose_acts_on_the_attach_time_rest_and_reattach_retakes_it(gpu):
    from rsd.frame import GpuScene, host_bvh, host_bvh_refit
    scene = _shape_scene("arcade_3000")
    nv = scene.positions.shape[0]
    rig = _rig(nv, nv // 3, "scattered", seed=9)
    A, _, _ = _poses(2)
    rng = np.random.default_rng(4)
    p1 = np.ascontiguousarray(scene.positions + (0.02 * rng.standard_normal(scene.positions.shape)).astype(np.float32))
    built, off = host_bvh(scene)
    gs = GpuScene(gpu, scene, dynamic=True)
    try:
        def check(p, what):
            have, _ = gs.export_bvh()
            assert np.array_equal(_u32(have), _u32(host_bvh_refit(built, off, scene.indices, p))), what

        gs.attach_rig(rig)
        gs.update_positions(p1)
        gs.update_pose(A)
        # animated vertices: from the rest taken at attach (the upload's positions); the others stay at P1
        check(skinning_checker.posed(p1, rig, A, rest=scene.positions[rig.vertex_ids]), "attach-time rest")
        gs.update_positions(p1)
        gs.attach_rig(rig)
        gs.update_pose(A)
        check(skinning_checker.posed(p1, rig, A), "re-attached: P1 is the rest")
        # a rig that brings its own rest positions
        own = scene.positions[rig.vertex_ids] * np.float32(0.5)
        rig2 = type(rig)(rig.vertex_ids, rig.matrix_ids, rig.weights, rig.matrix_count, rest=own)
        gs.attach_rig(rig2)
        gs.update_pose(A)
        check(skinning_checker.posed(p1, rig2, A), "the rig's own rest")
    finally:
        gs.release()


@pytest.fixture(scope="module")
def parity(gpu):
    """arcade_3000 with the vertices of its last eighth of triangles rigged to 3 matrices, posed on the GPU; the same
    positions from the checker uploaded fresh and static."""
    from rsd.animation import Rig
    from rsd.frame import GpuScene, Renderer
    scene = _shape_scene("arcade_3000")
    ids = np.unique(scene.indices[-max(1, scene.indices.shape[0] // 8):]).astype(np.uint32)
    m = np.zeros((ids.size, 4), np.uint32)
    m[:, 0], m[:, 1] = ids % 3, (ids + 1) % 3
    w = np.zeros((ids.size, 4), np.float32)
    w[:, 0] = 1.0
    w[1::2] = (0.5, 0.5, 0, 0)  # every other vertex is blended between two matrices
    rig = Rig(ids, m, w, 3)
    M = skinning_checker.identity_matrices(3)
    c, s = np.cos(0.2), np.sin(0.2)
    M[0] = np.float32([c, 0, s, 0.4, 0, 1, 0, 0.3, -s, 0, c, -0.5])
    M[1] = np.float32([1, 0, 0, 0.45, 0, 1.1, 0, 0.25, 0, 0, 1, -0.4])
    M[2] = np.float32([1, 0, 0, 0.35, 0, c, -s, 0.35, 0, s, c, -0.55])
    moved = dataclasses.replace(scene, positions=skinning_checker.posed(scene.positions, rig, M))
    dyn = GpuScene(gpu, scene, dynamic=True)
    dyn.attach_rig(rig)
    fresh, static = GpuScene(gpu, moved), GpuScene(gpu, scene)

    def frame(sc, gs):
        r = Renderer(sc, _cfg(sd_samples=4), dev=gpu, gpu_scene=gs)
        r.gbuffer()
        r.frame()
        return r, r.numpy()

    dyn.update_pose(M)
    stale = dyn.dynamic_info().entry_grid_current
    r, posed_frame = frame(moved, dyn)
    out = dict(r=r, posed=posed_frame, fresh=frame(moved, fresh)[1], old=frame(scene, static)[1], moved=moved, dyn=dyn,
               stale=stale, frame=frame)
    yield out
    for g in (dyn, fresh, static):
        g.release()


KEYS = ["depth", "normals", "ray_min", "ray_max", "sd", "ao"]


@pytest.mark.parametrize("key", KEYS)
def test_posed_scene_renders_like_a_fresh_upload(parity, key):
    a, b = parity["posed"][key], parity["fresh"][key]
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), key
    if key in ("depth", "sd", "ao"):
        assert a.tobytes() != parity["old"][key].tobytes(), "the pose does not show in this output"


def test_posed_scene_matches_the_oracle(oracle, parity):
    O, g, r, moved = oracle, parity["posed"], parity["r"], parity["moved"]
    osc = O.Scene(moved.positions, moved.indices, moved.flags)
    o = oracle_frame(O, osc, to_oracle(r.cam, O.Camera), to_oracle(r.vao, O.VAOData), to_oracle(r.sdp, O.SDParams),
                     to_oracle(r.svp, O.SVAOParams), W, H, r.sd_w, r.sd_h)
    assert o["stats"][0] > 100, "hardly any live SD ray: the frame is degenerate"
    assert np.array_equal(_u32(g["depth"]), _u32(o["depth"]))
    assert np.array_equal(g["ray_min"], o["ray_min"]) and np.array_equal(g["ray_max"], o["ray_max"])
    assert np.array_equal(_u32(g["sd"]), _u32(o["sd"]))
    assert np.array_equal(g["ao"], o["ao"])


def test_a_pose_marks_the_entry_grid_stale_and_a_rebuild_keeps_the_bits(parity):
    dyn = parity["dyn"]
    assert dyn.info.entry_cells > 0 and parity["stale"] == 0
    dyn.rebuild_entry_grid()
    assert dyn.dynamic_info().entry_grid_current == 1
    _, again = parity["frame"](parity["moved"], dyn)
    for key in KEYS:
        assert again[key].tobytes() == parity["posed"][key].tobytes(), key


def test_bad_rigs_and_poses_are_refused_on_the_host(gpu):
    from rsd import abi
    from rsd.animation import Rig
    from rsd.frame import GpuScene
    scene = _shape_scene("grid_24")
    nv = scene.positions.shape[0]
    one = np.float32([[1, 0, 0, 0]])
    I2 = skinning_checker.identity_matrices(2)

    def refused(gs, rig, match):
        with pytest.raises(abi.RsdError, match=match) as e:
            gs.attach_rig(rig)
        assert e.value.status == abi.ERR_INVALID_ARG

    static, dyn = GpuScene(gpu, scene), GpuScene(gpu, scene, dynamic=True)
    try:
        refused(static, Rig([0], [[0, 0, 0, 0]], one, 1), "not dynamic")
        with pytest.raises(abi.RsdError, match="not dynamic"):
            static.update_pose(I2)
        with pytest.raises(abi.RsdError, match="no rig") as e:
            dyn.update_pose(I2)
        assert e.value.status == abi.ERR_INVALID_ARG
        refused(dyn, Rig([3, 5, 3], np.zeros((3, 4)), np.tile(one, (3, 1)), 2), "named twice")
        refused(dyn, Rig([3], [[0, 0, 2, 0]], one, 2), "matrix id")
        refused(dyn, Rig([nv], [[0, 0, 0, 0]], one, 2), "vertex id")
        refused(dyn, Rig([3], [[0, 0, 0, 0]], one, 0), "matrix_count")
        assert dyn.rig_info().attached == 0 and dyn.dynamic_info().updates == 0
        dyn.attach_rig(Rig([3], [[0, 1, 0, 0]], one, 2))
        with pytest.raises(abi.RsdError, match="matrix_count") as e:
            dyn.update_pose(skinning_checker.identity_matrices(3))
        assert e.value.status == abi.ERR_INVALID_ARG
        info = dyn.dynamic_info()
        assert info.updates == 0 and info.entry_grid_current == 1
        bvh, _ = dyn.export_bvh()
        assert np.array_equal(_u32(bvh), _u32(static.export_bvh()[0])), "a refused call moves nothing"
        # a rig that moves nothing is legal
        dyn.attach_rig(Rig([], np.zeros((0, 4)), np.zeros((0, 4)), 0))
        dyn.update_pose(np.zeros((0, 12), np.float32))
        assert dyn.dynamic_info().updates == 1
        assert np.array_equal(_u32(dyn.export_bvh()[0]), _u32(bvh))
    finally:
        static.release()
        dyn.release()


def test_gpu_scene_attaches_the_scenes_own_rig_and_animates(gpu):
    """GpuScene(dynamic=True) on a built animated scene: animate(t) leaves the checker's positions at the controller's
    matrices; at the rest time those are the soup."""
    from conftest import ROOT
    from rsd.frame import GpuScene, host_bvh, host_bvh_refit
    from rsd.pyscene import load_pyscene
    scene = load_pyscene(ROOT / "tests" / "fixtures" / "turnstile.pyscene").build("turnstile")
    built, off = host_bvh(scene)
    gs = GpuScene(gpu, scene, dynamic=True)
    try:
        assert gs.rig is scene.rig and gs.rig_info().count == scene.rig.count == 96
        for t in (0.37, 0.0):
            gs.animate(t)
            p = skinning_checker.posed(scene.positions, scene.rig, scene.rig.matrices(t))
            have, _ = gs.export_bvh()
            assert np.array_equal(_u32(have), _u32(host_bvh_refit(built, off, scene.indices, p))), t
        assert p.tobytes() == scene.positions.tobytes() and np.array_equal(_u32(have), _u32(built))
    finally:
        gs.release()


# ------------------------------------------------------------------ the float mode of the pose kernel
# csrc/skinning.hip is an exact kernel: every product and sum rounded on its own, denormals kept, non-finite values
# propagated.  The inputs above are all of order 1; these are not.  Bytes only: no frame is rendered.

TINY = np.finfo(np.float32).tiny


@pytest.fixture(params=["global", "lds"])
def table_variant(request):
    prev = os.environ.get("RSD_POSE_TABLE")
    os.environ["RSD_POSE_TABLE"] = request.param
    yield request.param
    if prev is None:
        del os.environ["RSD_POSE_TABLE"]
    else:
        os.environ["RSD_POSE_TABLE"] = prev


def _edge_rig(scene, rest):
    base = _rig(scene.positions.shape[0], BLOCK + 1, "scattered", seed=31)
    assert np.isin(base.vertex_ids, scene.indices).all(), "every rig vertex reads back from a triangle record"
    return type(base)(base.vertex_ids, base.matrix_ids, base.weights, NM, rest=np.ascontiguousarray(rest, np.float32))


def _signed(rng, lo, hi, shape):
    return rng.choice([-1.0, 1.0], shape) * rng.uniform(lo, hi, shape)


def _pose_and_read(gpu, scene, rig, M):
    from rsd.frame import GpuScene
    gs = GpuScene(gpu, scene, dynamic=True)
    try:
        gs.attach_rig(rig)
        gs.update_pose(M)
        return morph_checker.export_positions(gs, scene.indices), gs.export_bvh()[0]
    finally:
        gs.release()


def test_pose_keeps_denormal_results(gpu, table_variant):
    """Matrix entries of about 1e-25 and rest coordinates of about 1e-15: the blended products lie near 1e-40.
    Matrices 0 .. 2 carry denormal translations, 3 and 4 normal ones, so the expected words are of both kinds -- counted
    on the checker's output before the GPU is looked at (a numpy that flushed denormals fails here, and so it should).
    A build of this file that flushed float32 denormals would store zeros where the checker has 1e-40."""
    from rsd.frame import host_bvh, host_bvh_refit
    scene = _shape_scene("arcade_3000")
    rng = np.random.default_rng(40)
    rig = _edge_rig(scene, _signed(rng, 0.5e-15, 2e-15, (BLOCK + 1, 3)))
    M = (skinning_checker.random_matrices(rng, NM).astype(np.float64) * 1e-25).astype(np.float32)
    M[:3, [3, 7, 11]] = _signed(rng, 1e-42, 9e-41, (3, 3)).astype(np.float32)
    want = skinning_checker.posed(scene.positions, rig, M)
    mag = np.abs(want[rig.vertex_ids].astype(np.float64))
    denormal, normal = (mag > 0) & (mag < TINY), (mag >= TINY) & np.isfinite(mag)
    assert denormal.sum() >= 32 and normal.sum() >= 32, (denormal.sum(), normal.sum())
    have, bvh = _pose_and_read(gpu, scene, rig, M)
    ref = np.unique(scene.indices)
    bad = np.flatnonzero((_u32(have[ref]) != _u32(want[ref])).any(axis=1))
    assert bad.size == 0, (bad.size, ref[bad[:4]], have[ref[bad[:4]]], want[ref[bad[:4]]])
    built, off = host_bvh(scene)
    assert np.array_equal(_u32(bvh), _u32(host_bvh_refit(built, off, scene.indices, want)))


def test_pose_overflows_to_both_infinities(gpu, table_variant):
    """One matrix carries 3e38 on its diagonal: where its weights sum past 1 the blend overflows, and where the rest
    coordinate is above 1.14 the product does.  One huge entry per row and no zero rest coordinate: no inf - inf and no
    0 * inf, so the expected words hold both infinities and no NaN, and the comparison is bitwise throughout."""
    from rsd.frame import host_bvh, host_bvh_refit
    scene = _shape_scene("arcade_3000")
    rng = np.random.default_rng(41)
    rig = _edge_rig(scene, _signed(rng, 1.3, 2.0, (BLOCK + 1, 3)))
    M = skinning_checker.random_matrices(rng, NM)
    M[NM - 1] = np.float32([3e38, 0.5, 0.25, 0.1, 0.3, -3e38, 0.2, 0.1, 0.1, 0.2, 3e38, 0.0])
    with np.errstate(over="ignore"):
        want = skinning_checker.posed(scene.positions, rig, M)
    out = want[rig.vertex_ids]
    assert np.isposinf(out).any() and np.isneginf(out).any() and not np.isnan(out).any() and np.isfinite(out).sum() >= 32
    have, bvh = _pose_and_read(gpu, scene, rig, M)
    ref = np.unique(scene.indices)
    bad = np.flatnonzero((_u32(have[ref]) != _u32(want[ref])).any(axis=1))
    assert bad.size == 0, (bad.size, ref[bad[:4]], have[ref[bad[:4]]], want[ref[bad[:4]]])
    built, off = host_bvh(scene)
    assert np.array_equal(_u32(bvh), _u32(host_bvh_refit(built, off, scene.indices, want)))


def test_pose_propagates_a_nan_weight_and_an_infinite_rest(gpu, table_variant):
    """Rig vertex 5 has a NaN weight, rig vertex 9 an infinite rest coordinate.  Everything is compared bit for bit
    with the checker except the six words of those two vertices where the checker holds a NaN: there the kernel must
    hold a NaN too, of whatever payload (numpy on the host generates the negative default NaN for inf - inf and
    0 * inf, the GPU the positive one).  The tree is rsd_bvh_refit's at the checker's positions with those NaN words
    in the device's payload."""
    from rsd.frame import host_bvh, host_bvh_refit
    scene = _shape_scene("arcade_3000")
    rng = np.random.default_rng(42)
    rest = _signed(rng, 0.5, 2.0, (BLOCK + 1, 3))
    rest[9, 2] = np.inf
    rig = _edge_rig(scene, rest)
    rig.weights[5, 1] = np.nan
    A, _, _ = _poses(13)
    with np.errstate(invalid="ignore"):
        want = skinning_checker.posed(scene.positions, rig, A)
    special = rig.vertex_ids[[5, 9]]
    nan = np.isnan(want)
    assert nan[special[0]].all() and not np.isfinite(want[special[1]]).any() and nan.sum() == nan[special].sum()
    have, bvh = _pose_and_read(gpu, scene, rig, A)
    ref = np.unique(scene.indices)
    assert np.array_equal(np.isnan(have[ref]), nan[ref]), "NaN exactly where the checker has one"
    same = _u32(have) == _u32(want)
    assert (same | nan)[ref].all(), "every other word bit for bit"
    at = want.copy()
    at[nan] = have[nan]
    built, off = host_bvh(scene)
    assert np.array_equal(_u32(bvh), _u32(host_bvh_refit(built, off, scene.indices, at)))
