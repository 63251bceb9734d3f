"""The BVH refit on the host (rsd_bvh_refit, csrc/bvh_refit.h): the byte-exact statement of what an update of a
dynamic scene leaves on the device (tests/test_gpu_scene_update.py compares the kernels with it).

Checked against tests/bvh_refit_checker.py, which recomputes every slot's box from the records with numpy's float
min / max and nextafter: identity (a refit to the unchanged positions is the build, byte for byte), moved positions
(every box and record as recomputed, every ref / cnt / prim / flags word untouched), the return trip, the shapes at
which the tree degenerates, and the refusals.  tests/native/check_bvh_refit.cpp runs the same code under
AddressSanitizer and UBSan, with a real spatial-split tree among its cases."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import scenes_adversarial
from bvh_refit_checker import expected_refit, layout, topology_words

HERE = Path(__file__).resolve().parent
CSRC = HERE.parent / "ray-traced-stochastic-depth-map_amd" / "csrc"


def _scene(name):
    from rsd.ingest import load_obj
    from rsd.scenes import Scene, make_scene
    cam = dict(pos=[0.0, 0.0, 3.0], target=[0.0, 0.0, 0.0], up=[0.0, 1.0, 0.0])
    if name == "one_triangle":  # a leaf root: one wide node with one leaf child
        return Scene(name, np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], np.float32), np.array([[0, 1, 2]], np.uint32),
                     np.zeros(1, np.uint32), cam)
    if name == "five_triangles":  # more than one leaf's worth: a root with several leaf children
        p = np.array([[x, y, 0.25 * x * y] for y in range(3) for x in range(4)], np.float32)
        t = np.array([[0, 1, 4], [1, 5, 4], [2, 3, 6], [5, 6, 9], [6, 7, 11]], np.uint32)
        return Scene(name, p, t, np.zeros(5, np.uint32), cam)
    if name == "grid_24":  # more than the root's four leaves hold: the first inner child
        p = np.array([[x, y, 0.25 * x * y] for y in range(4) for x in range(5)], np.float32)
        i = np.arange(20).reshape(4, 5)
        a, b, c, d = i[:-1, :-1], i[:-1, 1:], i[1:, 1:], i[1:, :-1]
        t = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 2).reshape(-1, 3).astype(np.uint32)
        return Scene(name, p, np.ascontiguousarray(t), np.zeros(24, np.uint32), cam)
    if name == "slivers":  # long needles, overlapping boxes: the deepest tree of the adversarial scenes
        return scenes_adversarial.make("slivers")
    if name == "crate":
        return load_obj(HERE / "fixtures" / "crate.obj").build("crate")
    if name == "arcade_3000":
        return make_scene("arcade_tiny", target_tris=3000)
    raise KeyError(name)


SCENES = ["one_triangle", "five_triangles", "grid_24", "slivers", "crate", "arcade_3000"]


def _motion(name, scene):
    p = scene.positions.astype(np.float32).copy()
    rng = np.random.default_rng(7)
    nv = p.shape[0]
    if name == "subset_translated":
        p[: max(1, nv // 3)] += np.float32([0.3, -0.2, 0.5])
    elif name == "jitter":
        p += (0.01 * rng.standard_normal(p.shape)).astype(np.float32)
    elif name == "far_outside":  # one part leaves the original root box by far
        tri = scene.indices[: max(1, scene.indices.shape[0] // 8)]
        p[np.unique(tri)] += np.float32([1000.0, 2000.0, -3000.0])
    elif name == "collapsed":  # triangle 0 becomes a point
        p[scene.indices[0]] = p[scene.indices[0][0]]
    elif name == "denormal_mixed_sign":  # coordinates of denormal size on both sides of zero, and zeros of both signs
        p = ((p - p.mean(axis=0, dtype=np.float64)).astype(np.float64) * 1e-41).astype(np.float32)
        p[scene.indices[0][0]] = [0.0, -0.0, 1e-45]
        assert (np.abs(p[p != 0]) < np.finfo(np.float32).tiny).any() and (p < 0).any() and (p > 0).any()
    else:
        raise KeyError(name)
    return p


MOTIONS = ["subset_translated", "jitter", "far_outside", "collapsed", "denormal_mixed_sign"]


@pytest.fixture(scope="module")
def built():
    from rsd.frame import host_bvh
    cache = {}

    def get(name):
        if name not in cache:
            s = _scene(name)
            cache[name] = (s,) + host_bvh(s)
        return cache[name]
    return get


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", SCENES)
def test_identity_refit_reproduces_the_build(built, name):
    """Unchanged positions: nodes, records and the pad, over the whole allocation."""
    from rsd.frame import host_bvh_refit
    scene, bvh, off = built(name)
    _, nn, nrec = layout(bvh, off)
    assert nrec == scene.indices.shape[0] and nn >= 1
    out = host_bvh_refit(bvh, off, scene.indices, scene.positions)
    assert out.nbytes == bvh.nbytes and np.array_equal(_u32(out), _u32(bvh))
    assert np.array_equal(expected_refit(bvh, off, scene.indices, scene.positions), _u32(bvh)), "the checker itself"


def test_the_small_shapes_are_the_ones_meant(built):
    _, bvh, off = built("one_triangle")
    w, nn, _ = layout(bvh, off)
    assert nn == 1 and list(w[28:32]) == [1, 0, 0, 0] and list(w[25:28]) == [0xFFFFFFFF] * 3
    _, bvh, off = built("five_triangles")
    w, nn, _ = layout(bvh, off)
    assert nn == 1 and (w[28:32] != 0).sum() >= 2, "one node, several leaf children"
    _, bvh, off = built("grid_24")
    w, nn, _ = layout(bvh, off)
    nodes = w[:32 * nn].reshape(nn, 8, 4)
    assert nn >= 2 and ((nodes[0, 7] == 0) & (nodes[0, 6] != 0xFFFFFFFF)).any(), "the root has an inner child"


@pytest.mark.parametrize("motion", MOTIONS)
@pytest.mark.parametrize("name", SCENES)
def test_moved_positions_match_the_checker(built, name, motion):
    from rsd.frame import host_bvh_refit
    scene, bvh, off = built(name)
    p1 = _motion(motion, scene)
    out = host_bvh_refit(bvh, off, scene.indices, p1)
    want = expected_refit(bvh, off, scene.indices, p1)
    bad = np.flatnonzero(_u32(out) != want)
    assert bad.size == 0, (name, motion, bad[:8], _u32(out)[bad[:8]], want[bad[:8]])
    assert np.array_equal(topology_words(out, off), topology_words(bvh, off))
    if motion != "collapsed" or scene.indices.shape[0] > 1:
        assert not np.array_equal(_u32(out), _u32(bvh)), "the motion moved nothing"


@pytest.mark.parametrize("name", SCENES)
def test_return_trip_reproduces_the_build(built, name):
    from rsd.frame import host_bvh_refit
    scene, bvh, off = built(name)
    there = host_bvh_refit(bvh, off, scene.indices, _motion("far_outside", scene))
    back = host_bvh_refit(there, off, scene.indices, scene.positions)
    assert np.array_equal(_u32(back), _u32(bvh))


def test_refit_in_place(built):
    from rsd import abi
    scene, bvh, off = built("crate")
    p1 = _motion("jitter", scene)
    buf = bvh.copy()
    ind = np.ascontiguousarray(scene.indices, np.uint32)
    abi.check(abi.lib().rsd_bvh_refit(buf.ctypes.data, buf.nbytes, off, ind.ctypes.data, ind.shape[0], p1.ctypes.data,
                                      p1.shape[0], buf.ctypes.data), "rsd_bvh_refit")
    assert np.array_equal(_u32(buf), expected_refit(bvh, off, scene.indices, p1))


def test_refusals(built):
    from rsd import abi
    L = abi.lib()
    scene, bvh, off = built("grid_24")
    ind = np.ascontiguousarray(scene.indices, np.uint32)
    pos = np.ascontiguousarray(scene.positions, np.float32)
    out = np.empty_like(bvh)
    call = lambda b, nbytes, o, i, nt, p, nv: L.rsd_bvh_refit(  # noqa: E731
        b.ctypes.data, nbytes, o, i.ctypes.data, nt, p.ctypes.data, nv, out.ctypes.data)
    assert call(bvh, bvh.nbytes, off, ind, 24, pos, pos.shape[0]) == abi.RSD_OK
    # wrong vertex_count: an index then points past the positions
    assert call(bvh, bvh.nbytes, off, ind, 24, pos, int(ind.max())) == abi.ERR_INVALID_ARG
    assert b"vertex_count" in L.rsd_last_error()
    # spatial splits: more records than triangles, or two records of one triangle
    assert call(bvh, bvh.nbytes, off, ind, 23, pos, pos.shape[0]) == abi.ERR_UNSUPPORTED
    assert b"spatial splits" in L.rsd_last_error()
    dup = bvh.copy()
    w = dup.view(np.uint32)
    w[4 * off + 12 + 3] = w[4 * off + 3]
    assert call(dup, dup.nbytes, off, ind, 24, pos, pos.shape[0]) == abi.ERR_UNSUPPORTED
    # bytes that are not a BVH of rsd_bvh_build
    assert call(bvh, bvh.nbytes - 4, off, ind, 24, pos, pos.shape[0]) == abi.ERR_INVALID_ARG
    loop = bvh.copy()
    w = loop.view(np.uint32)
    nn = off // 8
    inner = [(n, i) for n in range(nn) for i in range(4) if w[32 * n + 28 + i] == 0 and w[32 * n + 24 + i] != 0xFFFFFFFF]
    n, i = inner[0]
    w[32 * n + 24 + i] = n  # a child that is its own parent
    assert call(loop, loop.nbytes, off, ind, 24, pos, pos.shape[0]) == abi.ERR_INVALID_ARG
    assert L.rsd_bvh_refit(None, 0, 0, None, 0, None, 0, None) == abi.ERR_INVALID_ARG
    # the updates of a scene need a scene (and a dynamic one: tests/test_gpu_scene_update.py)
    assert L.rsd_scene_update_positions(None, pos.ctypes.data, pos.shape[0], 0, None) == abi.ERR_INVALID_ARG
    assert L.rsd_scene_update_subset(None, None, None, 0, None) == abi.ERR_INVALID_ARG
    assert L.rsd_scene_rebuild_entry_grid(None) == abi.ERR_INVALID_ARG
    assert L.rsd_scene_dynamic_info_get(None, None) == abi.ERR_INVALID_ARG
    assert L.rsd_graph_update_scene_positions(None, None, 0, 0, None) == abi.ERR_INVALID_ARG
    assert C.sizeof(abi.SceneDynamicInfo) == 24


def test_host_refit_under_sanitizers(tmp_path):
    """tests/native/check_bvh_refit.cpp: the host refit (and the builder under it) with AddressSanitizer and UBSan --
    identity, random motion against a float min / max + std::nextafter restatement, the bit steps against
    std::nextafter at the edges of the format, and the refusal of a real spatial-split tree."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path / "check_bvh_refit"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", f"-I{CSRC}", "-o", str(exe),
                    str(HERE / "native" / "check_bvh_refit.cpp"), str(CSRC / "bvh_refit_host.cpp"),
                    str(CSRC / "bvh_build.cpp"), "-pthread"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "failures 0", out.stdout
