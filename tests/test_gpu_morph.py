"""GPU: morph targets on the device (rsd_scene_attach_morph, rsd_scene_update_pose_morph, rsd_scene_morph_info_get;
csrc/skinning.hip pose_kernel<*, true>).

All comparisons are bitwise, against tests/morph_checker.py; the positions are read back from the device's triangle
records (morph_checker.export_positions).  The scene is a 43 x 7 grid of 301 vertices, every one named by a triangle: the
rig covers vertices 22 .. 278 (257: one lane of a second workgroup), so 22 vertices (66 floats) on each side of what a
pose writes are canaries that must keep their upload bits.  Every id handed to the device is valid: the refusals are
host checks."""
import os

import numpy as np
import pytest

import morph_checker
import skinning_checker

pytestmark = pytest.mark.gpu

F = np.float32
NX, NY, PAD = 43, 7, 22
NM = 4  # matrices


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rsd.frame import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def grid():
    from rsd.scenes import Scene
    rng = np.random.default_rng(41)
    p = np.array([[x, y, 0.0] for y in range(NY) for x in range(NX)], F)
    p[:, 2] = rng.uniform(0.5, 1.5, len(p)).astype(F)
    p[:, :2] += 0.25
    i = np.arange(NX * NY).reshape(NY, NX)
    a, b, c, d = i[:-1, :-1], i[:-1, 1:], i[1:, 1:], i[1:, :-1]
    t = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 2).reshape(-1, 3).astype(np.uint32)
    cam = dict(pos=[20.0, 3.0, 40.0], target=[20.0, 3.0, 0.0], up=[0.0, 1.0, 0.0])
    s = Scene("grid_301", p, np.ascontiguousarray(t), np.zeros(len(t), np.uint32), cam)
    assert s.positions.shape[0] == 301 == 2 * PAD + 257 and np.unique(t).size == 301
    return s


def _rig(scene, count, seed):
    """`count` vertices from PAD on, influences cycling through rigid, two and four weights; vertex 0 of the rig is
    rigid on matrix 0 with a rest x of -0 (the zero-sign case)."""
    from rsd.animation import Rig
    rng = np.random.default_rng(seed)
    ids = np.arange(PAD, PAD + count, dtype=np.uint32)
    m = rng.integers(0, NM, (count, 4)).astype(np.uint32)
    w = np.zeros((count, 4), F)
    for i in range(count):
        kind = i % 3
        if kind == 0:
            m[i], w[i] = (0 if i == 0 else m[i, 0], 0, 0, 0), (1, 0, 0, 0)
        elif kind == 1:
            w[i] = (0.75, 0, 0.5, 0)
        else:
            w[i] = (0.3, 0.2, 0.1, 0.3)
    rest = scene.positions[ids].copy()
    rest[0, 0] = F(-0.0)
    return Rig(ids, m, w, NM, rest=rest)


def _matrices(seed):
    """Matrix 0 keeps the sign of a zero x: row 0 is (1, -0, -0, -0)."""
    M = skinning_checker.random_matrices(np.random.default_rng(seed), NM, translation=0.5)
    M[0] = skinning_checker.identity_matrices(1)[0]
    M[0, 1:4] = F(-0.0)
    return M


def _table(count, weight_count, seed):
    """Entries per rig vertex cycle through 0, 1 and 9 (vertex 0: 1 entry, weight id 0, delta x < 0).  Weight 0 is
    -0.0; with more than one weight, weight 1 is exactly 0."""
    rng = np.random.default_rng(seed)
    n = np.array([(1, 0, 9)[i % 3] for i in range(count)])
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.uint32)
    ids = rng.integers(0, weight_count, int(off[-1])).astype(np.uint32)
    deltas = rng.uniform(-0.2, 0.2, (int(off[-1]), 3)).astype(F)
    ids[0], deltas[0] = 0, (-0.125, 0.0, 0.0)
    w = rng.uniform(-1.0, 1.5, weight_count).astype(F)
    w[0] = F(-0.0)
    if weight_count > 1:
        w[1] = F(0.0)
        if ids.size > 3:
            ids[3] = 1  # a weight that is exactly 0, evaluated
    from rsd.animation import MorphTable
    return MorphTable(off, ids, deltas, weight_count), w


def _readback(gs, scene):
    p = morph_checker.export_positions(gs, scene.indices)
    assert not np.isnan(p).any()
    return p


def _assert_canaries(p, scene):
    for sl in (slice(0, PAD), slice(PAD + 257, None)):
        assert p[sl].size >= 64 and _u32(p[sl]).tobytes() == _u32(scene.positions[sl]).tobytes(), "a canary vertex moved"


@pytest.fixture(params=["global", "lds"])
def table_variant(request):
    prev = os.environ.get("RSD_POSE_TABLE")
    os.environ["RSD_POSE_TABLE"] = request.param
    yield request.param
    if prev is None:
        del os.environ["RSD_POSE_TABLE"]
    else:
        os.environ["RSD_POSE_TABLE"] = prev


@pytest.mark.parametrize("count,weight_count", [(257, 300), (257, 1), (1, 1), (1, 300)])
def test_morph_pose_matches_the_checker_bitwise(gpu, grid, table_variant, count, weight_count):
    """Host weights, then device weights with another weight table and pose, then the first again, on one scene."""
    import torch
    from rsd.frame import GpuScene
    rig = _rig(grid, count, seed=5)
    morph, w0 = _table(count, weight_count, seed=9 + count + weight_count)
    w1 = (w0 * F(-0.5)).astype(F)
    A, B = _matrices(3), _matrices(4)
    gs = GpuScene(gpu, grid, dynamic=True)
    try:
        gs.attach_rig(rig)
        gs.attach_morph(morph)
        info = gs.morph_info()
        assert (info.attached, info.count, info.weight_count, info.entry_count) == (1, count, weight_count, morph.entry_count)
        assert info.morph_bytes >= 4 * (count + 1) + 16 * morph.entry_count + 4 * weight_count
        steps = [("host", A, w0, (A, w0)), ("device", B, w1, (torch.from_numpy(B).cuda(), torch.from_numpy(w1).cuda())),
                 ("host again", A, w0, (A, w0))]
        for k, (what, M, w, args) in enumerate(steps):
            gs.update_pose_morph(*args)
            want = morph_checker.posed(grid.positions, rig, M, morph.offsets, morph.weight_ids, morph.deltas, w)
            have = _readback(gs, grid)
            bad = np.flatnonzero((_u32(have) != _u32(want)).any(axis=1))
            assert bad.size == 0, (what, bad.size, bad[:8], have[bad[:2]], want[bad[:2]])
            _assert_canaries(have, grid)
            assert gs.dynamic_info().updates == k + 1
            if what == "host":
                # -0 (rest x) + (-0 * -0.125 = +0) = +0: the zero-weight entry is evaluated and shows in the sign
                plain = skinning_checker.posed(grid.positions, rig, M)
                assert _u32(plain)[PAD, 0] == 0x80000000 and _u32(want)[PAD, 0] == 0 and _u32(have)[PAD, 0] == 0
                assert not np.array_equal(_u32(want), _u32(plain))
        # rsd_scene_update_pose keeps the weights of the last morph call
        gs.update_pose(B)
        want = morph_checker.posed(grid.positions, rig, B, morph.offsets, morph.weight_ids, morph.deltas, w0)
        assert _u32(_readback(gs, grid)).tobytes() == _u32(want).tobytes()
        assert gs.dynamic_info().entry_grid_current == (0 if gs.info.entry_cells else 1)
    finally:
        gs.release()


def test_zero_weights_and_no_table_are_the_plain_pose(gpu, grid, table_variant):
    """(a) a table whose weights are all zero and whose deltas change nothing by the checker == update_pose without the
    table; (b) a scene without a table: the existing skinning checker's bits (the template flag changed nothing)."""
    from rsd.animation import MorphTable, Rig
    from rsd.frame import GpuScene
    base = _rig(grid, 257, seed=6)
    rest = grid.positions[base.vertex_ids].copy()  # no -0 in the rest: adding +0 changes no bit
    rig = Rig(base.vertex_ids, base.matrix_ids, base.weights, NM, rest=rest)
    morph, _ = _table(257, 7, seed=2)
    zeros = np.zeros(7, F)
    A = _matrices(8)
    plain = skinning_checker.posed(grid.positions, rig, A)
    same = morph_checker.posed(grid.positions, rig, A, morph.offsets, morph.weight_ids, morph.deltas, zeros)
    assert _u32(plain).tobytes() == _u32(same).tobytes(), "the checker says these deltas at weight 0 change nothing"
    with_table, without = GpuScene(gpu, grid, dynamic=True), GpuScene(gpu, grid, dynamic=True)
    try:
        without.attach_rig(rig)
        without.update_pose(A)
        assert without.morph_info().attached == 0
        p0 = _readback(without, grid)
        assert _u32(p0).tobytes() == _u32(plain).tobytes(), "without a table: the skinning checker's bits"
        _assert_canaries(p0, grid)
        with_table.attach_rig(rig)
        with_table.attach_morph(MorphTable(morph.offsets, morph.weight_ids, morph.deltas, 7))
        with_table.update_pose(A)  # the weights after attach are zeros
        assert _u32(_readback(with_table, grid)).tobytes() == _u32(p0).tobytes()
        with_table.update_pose_morph(A, zeros)
        assert _u32(_readback(with_table, grid)).tobytes() == _u32(p0).tobytes()
    finally:
        with_table.release()
        without.release()


def test_state_between_calls(gpu, grid):
    """A new rig drops the table; a table without entries detaches; the bytes are accounted for."""
    import ctypes as C
    from rsd import abi
    from rsd.animation import MorphTable
    from rsd.frame import GpuScene
    rig = _rig(grid, 257, seed=5)
    morph, w = _table(257, 5, seed=1)
    A = _matrices(3)
    gs = GpuScene(gpu, grid, dynamic=True)

    def device_bytes():
        d = abi.SceneInfo()
        abi.check(abi.lib().rsd_scene_info_get(gs.h, C.byref(d)), "rsd_scene_info_get")
        return d.device_bytes

    try:
        with pytest.raises(abi.RsdError, match="no rig") as e:
            gs.attach_morph(morph)
        assert e.value.status == abi.ERR_INVALID_ARG
        gs.attach_rig(rig)
        with pytest.raises(abi.RsdError, match="no morph table"):
            gs.update_pose_morph(A, w)
        b0 = device_bytes()
        gs.attach_morph(morph)
        mb = gs.morph_info().morph_bytes
        assert mb > 0 and device_bytes() == b0 + mb
        gs.update_pose_morph(A, w)
        gs.attach_rig(rig)
        info = gs.morph_info()
        assert (info.attached, info.count, info.weight_count, info.entry_count, info.morph_bytes) == (0, 0, 0, 0, 0)
        assert device_bytes() == b0
        gs.update_pose(A)
        p = _readback(gs, grid)
        assert _u32(p).tobytes() == _u32(skinning_checker.posed(grid.positions, rig, A)).tobytes()
        gs.attach_morph(morph)
        gs.attach_morph(MorphTable(np.zeros(258, np.uint32), [], np.zeros((0, 3)), 5))
        assert gs.morph_info().attached == 0 and device_bytes() == b0
    finally:
        gs.release()


def test_bad_tables_are_refused_and_the_scene_still_poses(gpu, grid):
    from rsd import abi
    from rsd.animation import MorphTable
    from rsd.frame import GpuScene
    rig = _rig(grid, 257, seed=5)
    morph, w = _table(257, 5, seed=1)
    A = _matrices(3)
    gs = GpuScene(gpu, grid, dynamic=True)

    def refused(table, match):
        with pytest.raises(abi.RsdError, match=match) as e:
            gs.attach_morph(table)
        assert e.value.status == abi.ERR_INVALID_ARG

    try:
        gs.attach_rig(rig)
        gs.attach_morph(morph)
        off = morph.offsets.copy()
        off[11], off[12] = off[12], off[11]  # rig vertex 11 has nine entries: offsets[11] > offsets[12] afterwards
        assert off[11] > off[12]
        bad = MorphTable(morph.offsets, morph.weight_ids, morph.deltas, 5)
        bad.offsets = off
        refused(bad, "offsets decrease at rig vertex 11")
        ids = morph.weight_ids.copy()
        ids[7] = 5
        refused(MorphTable(morph.offsets, ids, morph.deltas, 5), "weight id 5 is out of range of weight_count 5")
        short, _ = _table(256, 5, seed=1)
        refused(short, "count 256 is not the rig's 257")
        first = morph.offsets.copy()
        first[0] = 1
        bad = MorphTable(morph.offsets, morph.weight_ids, morph.deltas, 5)
        bad.offsets = first
        refused(bad, r"offsets\[0\]")
        with pytest.raises(abi.RsdError, match="weight_count 4") as e:
            gs.update_pose_morph(A, w[:4])
        assert e.value.status == abi.ERR_INVALID_ARG
        info = gs.morph_info()
        assert (info.attached, info.entry_count) == (1, morph.entry_count) and gs.dynamic_info().updates == 0
        gs.update_pose_morph(A, w)
        have = _readback(gs, grid)
        want = morph_checker.posed(grid.positions, rig, A, morph.offsets, morph.weight_ids, morph.deltas, w)
        assert _u32(have).tobytes() == _u32(want).tobytes()
        _assert_canaries(have, grid)
    finally:
        gs.release()


# ------------------------------------------------------------------ the float mode of pose_kernel<*, true>
# The inputs above are of order 1.  Here the products w * delta are denormal, overflow, or carry a NaN; bytes only.

TINY = np.finfo(F).tiny


def _signed(rng, lo, hi, shape):
    return rng.choice([-1.0, 1.0], shape) * rng.uniform(lo, hi, shape)


def _edge_rig(grid, rest):
    from rsd.animation import Rig
    base = _rig(grid, 257, seed=5)
    return Rig(base.vertex_ids, base.matrix_ids, base.weights, NM, rest=np.ascontiguousarray(rest, F))


def _pose_morph_and_read(gpu, grid, rig, morph, M, w):
    from rsd.frame import GpuScene
    gs = GpuScene(gpu, grid, dynamic=True)
    try:
        gs.attach_rig(rig)
        gs.attach_morph(morph)
        gs.update_pose_morph(M, w)
        return morph_checker.export_positions(gs, grid.indices), gs.export_bvh()[0]
    finally:
        gs.release()


def _refit_bytes(grid, positions):
    from rsd.frame import host_bvh, host_bvh_refit
    built, off = host_bvh(grid)
    return host_bvh_refit(built, off, grid.indices, positions)


def test_morph_keeps_denormal_products(gpu, grid, table_variant):
    """Weights and deltas of about 1e-20 on rest coordinates of about 1e-39: every product w * delta is denormal and
    so is the sum it is added to.  Matrices 0 and 1 have no translation, so their vertices stay denormal through the
    pose; 2 and 3 give normal words.  Counted on the checker's output first; a build that flushed float32 denormals
    would add zeros and pose zeros."""
    from rsd.animation import MorphTable
    rng = np.random.default_rng(50)
    rig = _edge_rig(grid, _signed(rng, 1e-39, 9e-39, (257, 3)))
    base, _ = _table(257, 7, seed=3)
    deltas = _signed(rng, 0.5e-20, 2e-20, base.deltas.shape).astype(F)
    morph = MorphTable(base.offsets, base.weight_ids, deltas, 7)
    w = _signed(rng, 0.5e-20, 2e-20, 7).astype(F)
    M = skinning_checker.random_matrices(rng, NM, translation=0.5)
    M[:2, [3, 7, 11]] = 0
    want = morph_checker.posed(grid.positions, rig, M, morph.offsets, morph.weight_ids, morph.deltas, w)
    plain = skinning_checker.posed(grid.positions, rig, M)
    assert (_u32(want) != _u32(plain)).sum() >= 32, "the denormal products show in the result"
    mag = np.abs(want[rig.vertex_ids].astype(np.float64))
    denormal, normal = (mag > 0) & (mag < TINY), (mag >= TINY) & np.isfinite(mag)
    assert denormal.sum() >= 32 and normal.sum() >= 32, (denormal.sum(), normal.sum())
    have, bvh = _pose_morph_and_read(gpu, grid, rig, morph, M, w)
    bad = np.flatnonzero((_u32(have) != _u32(want)).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:8], have[bad[:2]], want[bad[:2]])
    _assert_canaries(have, grid)
    assert np.array_equal(_u32(bvh), _u32(_refit_bytes(grid, want)))


def test_morph_overflows_to_both_infinities(gpu, grid, table_variant):
    """Weight 2 is 3e38 and its deltas are (+-2, 0.01, 0.01), one sign per vertex: x overflows to that infinity, y and
    z stay finite, no inf - inf arises, and no blended matrix has a zero in column 0.  Both infinities and no NaN in
    the expected words; the comparison is bitwise throughout."""
    from rsd.animation import MorphTable
    rng = np.random.default_rng(51)
    rig = _edge_rig(grid, grid.positions[PAD:PAD + 257])
    base, w = _table(257, 7, seed=4)
    owner = np.repeat(np.arange(257), np.diff(base.offsets.astype(np.int64)))
    deltas = base.deltas.copy()
    big = base.weight_ids == 2
    assert big.sum() >= 32
    deltas[big] = np.stack([np.where(owner[big] % 2 == 0, 2.0, -2.0), np.full(big.sum(), 0.01),
                            np.full(big.sum(), 0.01)], 1).astype(F)
    morph = MorphTable(base.offsets, base.weight_ids, deltas, 7)
    w = w.copy()
    w[2] = F(3e38)
    M = skinning_checker.random_matrices(rng, NM, translation=0.5)
    with np.errstate(over="ignore"):
        want = morph_checker.posed(grid.positions, rig, M, morph.offsets, morph.weight_ids, morph.deltas, w)
    out = want[rig.vertex_ids]
    assert np.isposinf(out).any() and np.isneginf(out).any() and not np.isnan(out).any() and np.isfinite(out).sum() >= 32
    have, bvh = _pose_morph_and_read(gpu, grid, rig, morph, M, w)
    bad = np.flatnonzero((_u32(have) != _u32(want)).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:8], have[bad[:2]], want[bad[:2]])
    _assert_canaries(have, grid)
    assert np.array_equal(_u32(bvh), _u32(_refit_bytes(grid, want)))


def test_morph_propagates_a_nan_weight_and_an_infinite_rest(gpu, grid, table_variant):
    """Weight 6 is NaN and only the first entry of rig vertex 5 names it; rig vertex 9 has an infinite rest
    coordinate.  Bit for bit the checker's except the six words of those two vertices where the checker holds a NaN:
    there the kernel must hold a NaN too, of whatever payload (the host generates the negative default NaN for
    inf - inf and 0 * inf, the GPU the positive one).  The tree is rsd_bvh_refit's at the checker's positions with
    those NaN words in the device's payload."""
    from rsd.animation import MorphTable
    rng = np.random.default_rng(52)
    rest = grid.positions[PAD:PAD + 257].copy()
    rest[9, 1] = np.inf
    rig = _edge_rig(grid, rest)
    base, w = _table(257, 7, seed=6)
    ids = base.weight_ids.copy()
    ids[ids == 6] = 5
    e = int(base.offsets[5])
    assert base.offsets[6] - base.offsets[5] == 9
    ids[e] = 6
    morph = MorphTable(base.offsets, ids, base.deltas, 7)
    w = w.copy()
    w[6] = F(np.nan)
    M = skinning_checker.random_matrices(rng, NM, translation=0.5)
    with np.errstate(invalid="ignore"):
        want = morph_checker.posed(grid.positions, rig, M, morph.offsets, morph.weight_ids, morph.deltas, w)
    special = rig.vertex_ids[[5, 9]]
    nan = np.isnan(want)
    assert nan[special[0]].all() and not np.isfinite(want[special[1]]).any() and nan.sum() == nan[special].sum()
    have, bvh = _pose_morph_and_read(gpu, grid, rig, morph, M, w)
    assert np.array_equal(np.isnan(have), nan), "NaN exactly where the checker has one"
    assert ((_u32(have) == _u32(want)) | nan).all(), "every other word bit for bit"
    _assert_canaries(have, grid)
    at = want.copy()
    at[nan] = have[nan]
    assert np.array_equal(_u32(bvh), _u32(_refit_bytes(grid, at)))
