"""CPU checks of the adversarial-geometry scenes (tests/scenes_adversarial.py): the oracle's hit collection
(a BVH walk of its own) and its G-buffer are pinned to brute-force loops over all triangles
(tests/native/hits_ref.c, tests/native/depth_peel_ref.c) on every scene, and each scene is shown to force
what it was built for, on the references alone, so the GPU tests of tests/test_gpu_adversarial_walk.py
cannot pass vacuously."""
import shutil

import numpy as np
import pytest

import depth_peel_checker as DP
import hits_checker as HC
import scenes_adversarial as SA

pytestmark = pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")

W, H = HC.W, HC.H


@pytest.fixture(scope="session")
def hits_lib(oracle, tmp_path_factory):
    return HC.build(oracle, tmp_path_factory.mktemp("hits_ref"))


@pytest.fixture(scope="session")
def peel_lib(oracle, tmp_path_factory):
    return DP.build(oracle, tmp_path_factory.mktemp("depth_peel_ref"))


_cases = {}


def get_case(oracle, name):
    if name not in _cases:
        _cases[name] = HC.Case(oracle, name)
    return _cases[name]


@pytest.fixture
def case(oracle, request):
    return get_case(oracle, request.param)


every_scene = pytest.mark.parametrize("case", SA.NAMES, indirect=True)


def longest_tie(t, cnt):
    """Per texel the longest run of equal t among its (sorted) first CAP hits."""
    valid = np.arange(HC.CAP)[None, None, :] < cnt[..., None]
    same = (t[..., 1:] == t[..., :-1]) & valid[..., 1:]
    best = np.ones(cnt.shape, np.int64)
    run = np.ones(cnt.shape, np.int64)
    for k in range(same.shape[-1]):
        run = np.where(same[..., k], run + 1, 1)
        best = np.maximum(best, run)
    return np.where(cnt > 0, best, 0)


@every_scene
def test_oracle_hit_collection_is_brute_force(oracle, hits_lib, case):
    """KBuffer, N = 16, no normalisation, MAX_COUNT above every hit count: the oracle's map is the first 16
    t * cosT of the brute-force list per texel, DEFAULT_DEPTH beyond the count, bit for bit."""
    for cull in (1, 0):
        cnt, t, prim, zt = case.hits(oracle, hits_lib, cull)
        assert int(cnt.max()) < 1024
        sdp = case.sd_params(oracle, N=16, max_count=1024, impl=3, cull=cull)
        sd, stats = oracle.sd_trace(case.osc, case.ocam, sdp, case.depth, None, None, W, H)
        np.testing.assert_array_equal(HC.bits(sd), HC.bits(HC.first_depths(cnt, zt, 16)))
        assert int(stats[0]) == W * H and int(cnt.sum()) > 0
        # the list itself is in ascending (t, prim) order
        k = np.arange(HC.CAP - 1)[None, None, :] + 1 < np.minimum(cnt, HC.CAP)[..., None]
        a_t, b_t, a_p, b_p = t[..., :-1], t[..., 1:], prim[..., :-1], prim[..., 1:]
        assert (((a_t < b_t) | ((a_t == b_t) & (a_p < b_p))) | ~k).all()


@every_scene
def test_oracle_gbuffer_is_brute_force(oracle, peel_lib, case):
    """prev = 0, separation 0 discards nothing: the brute-force first layer is the oracle's G-buffer depth."""
    zero = np.zeros((H, W), np.float32)
    for cull in (0, 1, 2):
        want = oracle.gbuffer(case.osc, case.ocam, W, H, cull)[0]
        got = DP.peel(oracle, peel_lib, case, cull, zero, 0.0, 1, width=W, height=H)
        np.testing.assert_array_equal(DP.bits(got), DP.bits(want))


def test_layers_overflow_every_sorted_list(oracle, hits_lib):
    for name in ("layers", "layers_tight", "far_a_layers", "far_b_layers"):
        cnt = get_case(oracle, name).hits(oracle, hits_lib)[0]
        assert int(cnt.min()) >= 33, (name, int(cnt.min()))


def test_layers_tight_keys_are_nearly_equal(oracle, hits_lib):
    """The 40 layers lie within 117 ulps of depth: a texel's first 33 keys span less than 1e-4 of their value."""
    c = get_case(oracle, "layers_tight")
    cnt, t, _, _ = c.hits(oracle, hits_lib)
    assert ((t[..., 32] - t[..., 0]) < 1e-4 * t[..., 0]).all() and (t[..., 32] > t[..., 0]).all()


@pytest.mark.parametrize("name", ["coincident", "far_a_coincident", "far_b_coincident"])
def test_coincident_ties(oracle, hits_lib, name):
    c = get_case(oracle, name)
    cnt, t, prim, _ = c.hits(oracle, hits_lib)
    tie = longest_tie(t, cnt)
    assert (tie >= SA.COINCIDENT_COPIES).mean() >= 0.5, float((tie >= SA.COINCIDENT_COPIES).mean())


@pytest.mark.parametrize("name", ["axis_walls", "far_a_axis_walls", "far_b_axis_walls"])
def test_axis_walls_rays(oracle, hits_lib, name):
    """The centre ray has two zero direction components and starts in the planes of the partition and the
    shelf (flat boxes); every wall of the room is hit in at least one texel row."""
    c = get_case(oracle, name)
    sdp = c.sd_params(oracle)
    o, d, _, _, _ = oracle.sd_ray(c.ocam, sdp, c.depth, None, None, W, H, W // 2, H // 2)
    assert int((d == 0.0).sum()) == 2 and abs(float(d[2])) == 1.0
    pos = c.scene.positions
    assert (pos[:, 0] == o[0]).any() and (pos[:, 1] == o[1]).any()  # vertices on the camera's x and y planes
    for x in range(W):  # the centre column has d.x = 0, the centre row d.y = 0
        assert oracle.sd_ray(c.ocam, sdp, c.depth, None, None, W, H, x, H // 2)[1][1] == 0.0
    for y in range(H):
        assert oracle.sd_ray(c.ocam, sdp, c.depth, None, None, W, H, W // 2, y)[1][0] == 0.0
    cnt, _, prim, _ = c.hits(oracle, hits_lib, cull=0)
    valid = np.arange(HC.CAP)[None, None, :] < cnt[..., None]
    for wall, k in SA.AXIS_WALLS.items():
        on_wall = valid & (prim // SA.AXIS_WALL_TRIS == k)
        assert on_wall.any(axis=(1, 2)).sum() >= 1, wall


@pytest.mark.parametrize("name", ["grazing", "far_a_grazing", "far_b_grazing"])
def test_grazing_reciprocal_is_large(oracle, hits_lib, name):
    """The view axis meets the floor under 1 degree: |1 / d.y| > 57 on the centre row, whose rays hit the floor."""
    c = get_case(oracle, name)
    sdp = c.sd_params(oracle)
    d = oracle.sd_ray(c.ocam, sdp, c.depth, None, None, W, H, W // 2, H // 2)[1]
    assert 0.0 < abs(float(d[1])) < np.sin(np.radians(1.0))
    cnt, _, prim, _ = c.hits(oracle, hits_lib)
    assert (cnt[H // 2] >= 1).all() and (prim[H // 2, :, 0] < 2 * 24 * 24).all()


def test_slivers_spill_the_stack(oracle, hits_lib):
    """The modelled per-lane walk of the primary rays (the G-buffer's and the peel's rays) over librsd's own BVH
    leaves the 16-entry LDS stack on >= 64 rays and stays far below kStackTotal = 96; the walk it models finds
    the brute-force closest hit."""
    from rsd.frame import host_bvh
    c = get_case(oracle, "slivers")
    bvh, off = host_bvh(c.scene)
    for cull in (1, 0):
        mark, best_t, _ = HC.stack_model(oracle, hits_lib, c, bvh, off, cull)
        print("slivers, cull", cull, ": stack high-water mark", int(mark.min()), "..", int(mark.max()), ";",
              int((mark > 16).sum()), "rays above 16")
        assert int((mark > 16).sum()) >= 64
        assert int(mark.max()) < 64
        cnt, t, _, _ = c.hits(oracle, hits_lib, cull)
        np.testing.assert_array_equal(HC.bits(np.where(cnt > 0, t[..., 0], np.inf)), HC.bits(best_t))
    p, i = c.scene.positions, c.scene.indices
    area2 = np.linalg.norm(np.cross(p[i[:, 1]] - p[i[:, 0]], p[i[:, 2]] - p[i[:, 0]]), axis=1)
    assert int((area2 == 0).sum()) >= SA.SLIVER_COUNT // 20  # the triangles with two equal vertices


@pytest.mark.parametrize("name", ["layers", "coincident", "axis_walls", "far_b_layers", "far_b_coincident"])
def test_modelled_walk_finds_every_closest_key(oracle, hits_lib, name):
    """The modelled walk (librsd's box test restated in float32) ends with the brute-force closest key, primitive
    id included: a box test that drops the subtree of a tied hit shows here without a GPU."""
    from rsd.frame import host_bvh
    c = get_case(oracle, name)
    bvh, off = host_bvh(c.scene)
    _, best_t, best_p = HC.stack_model(oracle, hits_lib, c, bvh, off, 1)
    cnt, t, prim, _ = c.hits(oracle, hits_lib, 1)
    np.testing.assert_array_equal(HC.bits(np.where(cnt > 0, t[..., 0], np.inf)), HC.bits(best_t))
    np.testing.assert_array_equal(np.where(cnt > 0, prim[..., 0], np.uint32(0xffffffff)), best_p)
