"""The LBVH on the host (rsd_bvh_build_lbvh, csrc/lbvh.h): the byte-exact statement of what rsd_scene_rebuild_bvh
leaves on the device (tests/test_gpu_lbvh.py compares the kernels with it).

Checked against tests/lbvh_checker.py, a top-down numpy restatement of the definition that shares nothing with the
builder: the whole allocation byte for byte, at the upload's positions and at moved ones, on the refit tests' scenes,
on coincident triangles, on a planar scene and on a ~50 k-triangle scene.  Then what makes the bytes a tree librsd can
use: rsd_bvh_refit (which runs refit_topology) accepts it and is the identity on it, every primitive has one record,
leaves hold at most 4 triangles, the depth stays within the derived bound; the oracle's two tree-taking walks run on it.
tests/native/check_lbvh.cpp runs the builder under AddressSanitizer and UBSan."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lbvh_scenes
from bvh_refit_checker import EMPTY, layout
from helpers import to_oracle
from lbvh_checker import depth_bound, expected_lbvh

HERE = Path(__file__).resolve().parent
CSRC = HERE.parent / "ray-traced-stochastic-depth-map_amd" / "csrc"


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def built():
    """name -> (scene, LBVH bytes, tri_offset, checker words, checker depth), each computed once."""
    from rsd.frame import host_bvh_lbvh
    cache = {}

    def get(name):
        if name not in cache:
            s = lbvh_scenes.scene(name)
            want, woff, depth = expected_lbvh(s.positions, s.indices, s.flags)
            cache[name] = (s,) + host_bvh_lbvh(s) + (want, woff, depth)
        return cache[name]
    return get


def _wide_depth(w, nn):
    nodes = w[:32 * nn].reshape(nn, 8, 4)
    depth = np.zeros(nn, np.int64)
    depth[0] = 1
    for n in range(nn):  # a parent's index lies below its children's
        for i in range(4):
            if nodes[n, 7, i] == 0 and nodes[n, 6, i] != EMPTY:
                depth[nodes[n, 6, i]] = depth[n] + 1
    return int(depth.max())


@pytest.mark.parametrize("name", lbvh_scenes.SCENES)
def test_host_builder_matches_the_checker(built, name):
    scene, bvh, off, want, woff, _ = built(name)
    assert off == woff and bvh.nbytes == want.nbytes
    bad = np.flatnonzero(_u32(bvh) != want)
    assert bad.size == 0, (name, bad.size, bad[:8], _u32(bvh)[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("motion", ["moved", "large_motion"])
@pytest.mark.parametrize("name", lbvh_scenes.SMALL)
def test_moved_positions_match_the_checker(name, motion):
    import dataclasses
    from rsd.frame import host_bvh_lbvh
    s = lbvh_scenes.scene(name)
    p1 = lbvh_scenes.moved(s, 1) if motion == "moved" else lbvh_scenes.large_motion(s)
    bvh, off = host_bvh_lbvh(dataclasses.replace(s, positions=p1))
    want, woff, _ = expected_lbvh(p1, s.indices, s.flags)
    assert off == woff and np.array_equal(_u32(bvh), want), (name, motion)


@pytest.mark.parametrize("name", lbvh_scenes.SCENES)
def test_the_tree_is_one_a_refit_walks(built, name):
    """rsd_bvh_refit to the same positions: accepted (refit_topology: parents below children, one parent each, leaves
    inside the records) and the identity."""
    from rsd.frame import host_bvh_refit
    scene, bvh, off, *_ = built(name)
    out = host_bvh_refit(bvh, off, scene.indices, scene.positions)
    assert np.array_equal(_u32(out), _u32(bvh))


@pytest.mark.parametrize("name", lbvh_scenes.SCENES)
def test_records_leaves_and_depth(built, name):
    scene, bvh, off, _, _, want_depth = built(name)
    w, nn, nrec = layout(bvh, off)
    nt = scene.indices.shape[0]
    assert nrec == nt
    recs = w[4 * off:4 * off + 12 * nt].reshape(nt, 3, 4)
    assert np.array_equal(np.sort(recs[:, 0, 3]), np.arange(nt)), "every primitive in exactly one record"
    assert np.array_equal(recs[:, 1, 3], np.asarray(scene.flags, np.uint32)[recs[:, 0, 3]])
    nodes = w[:32 * nn].reshape(nn, 8, 4)
    cnt, ref = nodes[:, 7, :], nodes[:, 6, :]
    assert cnt.max() <= 4
    covered = np.zeros(nt, np.int64)
    for r, c in zip(ref[cnt > 0], cnt[cnt > 0]):
        covered[r:r + c] += 1
    assert (covered == 1).all(), "every record under exactly one leaf slot"
    used = (cnt > 0) | (ref != EMPTY)
    if nt > 4:
        assert (used.sum(axis=1) >= 2).all() and used[:, 0].all() and used[:, 1].all()
        assert ((used[:, 1:] <= used[:, :-1])).all(), "slots fill from 0 up"
    depth = _wide_depth(w, nn)
    assert depth == want_depth and depth <= depth_bound(nt), (depth, want_depth, depth_bound(nt))


def test_the_small_shapes_are_the_ones_meant(built):
    _, bvh, off, *_ = built("one_triangle")
    w, nn, _ = layout(bvh, off)
    assert nn == 1 and list(w[28:32]) == [1, 0, 0, 0] and list(w[24:28]) == [0] + [EMPTY] * 3
    _, bvh, off, *_ = built("five_triangles")
    w, nn, _ = layout(bvh, off)
    assert nn == 1 and sorted(w[28:32])[2:] in ([1, 4], [2, 3]), "five triangles: one node, two leaf slots"
    scene, bvh, off, *_ = built("coincident")
    w, nn, _ = layout(bvh, off)
    prim = w[4 * off:4 * off + 12 * 37].reshape(37, 3, 4)[:, 0, 3]
    assert np.array_equal(prim, np.arange(37)), "equal codes: the records are in primitive order"
    scene, bvh, off, *_ = built("planar")
    assert np.ptp(scene.positions[:, 2]) == 0 and layout(bvh, off)[1] > 4
    scene, bvh, off, *_ = built("arcade_50k")
    assert scene.indices.shape[0] > 40_000 and layout(bvh, off)[1] > 4000


def test_an_empty_scene():
    from rsd import abi
    desc = abi.SceneDesc(None, 0, None, 0, None)
    n, off = C.c_uint64(), C.c_uint32()
    buf = np.ones(32 + 48, np.uint32)
    assert abi.lib().rsd_bvh_build_lbvh(C.byref(desc), buf.ctypes.data, buf.nbytes, C.byref(n), C.byref(off)) == abi.RSD_OK
    assert n.value == buf.nbytes and off.value == 8
    assert list(buf[24:28]) == [EMPTY] * 4 and not buf[:24].any() and not buf[28:].any()


@pytest.mark.parametrize("walk", ["ordered", "wavefront"])
def test_the_oracle_walks_the_tree(oracle, built, walk):
    """The oracle takes a tree in its traversal-order and wavefront walks (its canonical trace builds its own): over the
    LBVH they trace the same rays as over the SAH tree, find hits, and touch the same texels."""
    from rsd.frame import FrameConfig, host_bvh, make_camera, make_vao, sd_params, svao_params
    O = oracle
    scene, bvh, off, *_ = built("arcade_3000")
    cfg = FrameConfig(visible_w=59, visible_h=29, guard_band=8, divisor=1, sd_guard_px=16, radius=2.0, numerics="exact",
                      hit_order=1 if walk == "ordered" else 2)
    cam, (vao, sd_w, sd_h) = to_oracle(make_camera(scene, cfg), O.Camera), make_vao(cfg)
    sdp, svp = to_oracle(sd_params(cfg, vao.sdGuard), O.SDParams), to_oracle(svao_params(cfg), O.SVAOParams)
    osc = O.Scene(scene.positions, scene.indices, scene.flags)
    z, n = O.gbuffer(osc, cam, cfg.fb_w, cfg.fb_h, sdp.cull_mode)
    _, _, rmin, rmax = O.svao_pass1(cam, to_oracle(vao, O.VAOData), svp, z, n, sd_w, sd_h)
    args = (cam, sdp, z, rmin, rmax, sd_w, sd_h)
    sah, soff = host_bvh(scene)
    w, nn, _ = layout(bvh, off)

    def run(tree, toff, depth):
        if walk == "ordered":
            return O.sd_trace_ordered(osc, tree, toff, *args)
        return O.sd_trace_wavefront(osc, tree, toff, min(208 - 3 * depth, 160), *args)

    sd_l, st_l = run(bvh, off, _wide_depth(w, nn))
    ws, ns, _ = layout(sah, soff)
    sd_s, st_s = run(sah, soff, _wide_depth(ws, ns))
    assert st_l[0] == st_s[0] > 100 and st_l[1] > 0
    # the streams differ in order only: a ray finds a hit over one tree exactly when it finds one over the other.  A
    # texel's samples stay at the clear value exactly where its ray accepted no hit.
    touched = lambda sd: (_u32(sd) != _u32(sd).ravel()[0]).reshape(sd.shape).any(axis=(0, 3))  # noqa: E731
    assert sd_l.shape == sd_s.shape
    assert np.array_equal(touched(sd_l), touched(sd_s))


def test_refusals():
    from rsd import abi
    L = abi.lib()
    s = lbvh_scenes.scene("grid_24")
    ind, pos = np.ascontiguousarray(s.indices, np.uint32), np.ascontiguousarray(s.positions, np.float32)
    n, off = C.c_uint64(), C.c_uint32()
    desc = abi.SceneDesc(pos.ctypes.data, pos.shape[0], ind.ctypes.data, ind.shape[0], None)
    assert L.rsd_bvh_build_lbvh(C.byref(desc), None, 0, C.byref(n), C.byref(off)) == abi.RSD_OK
    buf = np.zeros(n.value // 4, np.uint32)
    # capacity below the size
    assert L.rsd_bvh_build_lbvh(C.byref(desc), buf.ctypes.data, n.value - 4, C.byref(n), C.byref(off)) == abi.ERR_INVALID_ARG
    assert b"capacity" in L.rsd_last_error()
    # an index past the vertices
    short = abi.SceneDesc(pos.ctypes.data, int(ind.max()), ind.ctypes.data, ind.shape[0], None)
    assert L.rsd_bvh_build_lbvh(C.byref(short), None, 0, C.byref(n), C.byref(off)) == abi.ERR_INVALID_ARG
    assert b"vertex_count" in L.rsd_last_error()
    # more triangles than a primitive id and the walks' stacks allow: refused before anything is read
    huge = abi.SceneDesc(pos.ctypes.data, pos.shape[0], ind.ctypes.data, 1 << 30, None)
    assert L.rsd_bvh_build_lbvh(C.byref(huge), None, 0, C.byref(n), C.byref(off)) == abi.ERR_UNSUPPORTED
    assert b"too many triangles" in L.rsd_last_error()
    assert L.rsd_bvh_build_lbvh(None, None, 0, None, None) == abi.ERR_INVALID_ARG
    # the rebuild needs a scene (and a dynamic one: tests/test_gpu_lbvh.py)
    assert L.rsd_scene_rebuild_bvh(None) == abi.ERR_INVALID_ARG
    assert L.rsd_scene_rebuild_info_get(None, None) == abi.ERR_INVALID_ARG
    assert C.sizeof(abi.SceneRebuildInfo) == 24


def test_depth_bound_of_the_definition():
    assert depth_bound(5) == (30 + 3) // 2 + 1 and depth_bound(1 << 29) == 30 and depth_bound((1 << 30) - 1) == 31
    # 96 stack entries, 3 pushes per level: 32 levels, reached only past 2^33 triangles -- beyond 32-bit primitive ids
    assert depth_bound(1 << 33) == 32 and depth_bound((1 << 33) + 1) == 33


def test_host_builder_under_sanitizers(tmp_path):
    """tests/native/check_lbvh.cpp: the host builder (and the refit under it) with AddressSanitizer and UBSan on the
    degenerate shapes -- no triangle, one, four, five, coincident triangles, a planar and a collinear scene, denormal and
    huge coordinates, shared vertices -- each checked to be a tree (refit_topology) that holds every primitive once."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path / "check_lbvh"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", f"-I{CSRC}", "-o", str(exe),
                    str(HERE / "native" / "check_lbvh.cpp"), str(CSRC / "lbvh_host.cpp"),
                    str(CSRC / "bvh_refit_host.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "failures 0", out.stdout
