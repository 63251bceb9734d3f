"""GPU: the dynamic-scene kernels at their launch and float edges (csrc/lbvh.hip, csrc/bvh_refit.hip).

All statements are bitwise, against the host definitions rsd_bvh_build_lbvh and rsd_bvh_refit, which
tests/test_dynamic_edges.py pins to the numpy checkers on the same inputs (tests/dynamic_edge_scenes.py) together with
the proof that each input reaches its edge:
  * rebuild_bvh() on triangles that sit exactly on the quantiser's cell boundaries and one float32 beside them (the
    correctly rounded double division of lbvh_quantise on gfx950), on 176 000 triangles whose scene box is defined
    past scene_box_kernel's launch cap (its grid-stride loop), and on the small counts where the launches change shape;
  * refit and rebuild at denormal, huge, infinite, far, collapsed and unreferenced-outlier positions, and with a NaN
    a triangle names;
  * rsd_scene_update_subset at the edges of its contract: counts around a block, id order, duplicates, ids past the
    vertices;
  * rsd_scene_motion_begin_frame's copy at every 3 * nv mod 4.
The GPU's own output is never the reference."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest

import dynamic_edge_scenes as E
import morph_checker
import mvec_checker as MV
from helpers import assert_canaries_intact, canary
from test_gpu_lbvh import _same
from test_gpu_scene_update import H, W, _cfg, _u32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rsd.frame import Device
    d = Device(0)
    yield d
    d.close()


def _rebuild_and_compare(gs, scene, positions, what, again=True):
    """rebuild_bvh() leaves host_bvh_lbvh's bytes at `positions`; returns them."""
    from rsd.frame import host_bvh_lbvh
    want, woff = host_bvh_lbvh(dataclasses.replace(scene, positions=np.ascontiguousarray(positions, np.float32)))
    before = gs.rebuild_info().rebuilds
    gs.rebuild_bvh()
    have, off = gs.export_bvh()
    assert off == woff, (what, off, woff)
    _same(have, want, (what, "rebuild"))
    info = gs.rebuild_info()
    assert (info.rebuilds, info.node_count) == (before + 1, woff // 8)
    assert gs.info.node_count == woff // 8 and gs.info.triangle_count == scene.indices.shape[0]
    from test_lbvh import _wide_depth
    assert info.wide_depth == gs.info.wide_depth == _wide_depth(_u32(want), woff // 8)
    if again:
        gs.rebuild_bvh()
        have2, off2 = gs.export_bvh()
        assert off2 == woff and gs.rebuild_info().rebuilds == before + 2
        _same(have2, want, (what, "second rebuild"))
    return want, woff


# ---------------------------------------------------------------------------------------------- B1: rebuild

def test_rebuild_on_the_cell_boundaries(gpu):
    """lbvh_quantise on gfx950: 3 x 1023 triangles whose quotient is exactly k / 1024, and their float32 neighbours.
    A division one ulp low at an exactly representable quotient truncates to k - 1: another code, another record order,
    other bytes."""
    from rsd.frame import GpuScene
    scene, _ = E.cell_edges()
    gs = GpuScene(gpu, scene, dynamic=True)
    try:
        _rebuild_and_compare(gs, scene, scene.positions, "cell_edges")
    finally:
        gs.release()


def test_rebuild_past_the_scene_box_launch_cap(gpu):
    """scene_box_kernel's grid-stride loop: 3 * nt exceeds its 2048 x 256 lanes and the vertices that define the scene
    box are read on the second trip only.  A wrong stride or a single trip gives a smaller box and other codes."""
    from rsd.frame import GpuScene
    scene = E.soup_176k()
    assert 3 * scene.indices.shape[0] > 2048 * 256  # csrc/lbvh.hip scene_box_kernel's cap
    gs = GpuScene(gpu, scene, dynamic=True)
    try:
        _rebuild_and_compare(gs, scene, scene.positions, "soup_176k")
    finally:
        gs.release()


@pytest.mark.parametrize("nt", E.SMALL_COUNTS)
def test_small_counts_rebuild_and_refit(gpu, nt):
    """The leaf root with cnt > 1 (2 .. 4), a root half that splits again (6 .. 21), ni across a wave and a block:
    refit of the upload's tree, rebuild (twice), refit of the rebuilt tree."""
    from rsd.frame import GpuScene, host_bvh, host_bvh_refit
    scene = E.soup(nt)
    p1, p2 = E.jitter(scene, 3), E.jitter(scene, 4)
    built, off = host_bvh(scene)
    gs = GpuScene(gpu, scene, dynamic=True)
    try:
        gs.update_positions(p1)
        _same(gs.export_bvh()[0], host_bvh_refit(built, off, scene.indices, p1), (nt, "refit before a rebuild"))
        gs.update_positions(scene.positions)
        tree, toff = _rebuild_and_compare(gs, scene, scene.positions, nt)
        gs.update_positions(p2)
        _same(gs.export_bvh()[0], host_bvh_refit(tree, toff, scene.indices, p2), (nt, "refit after a rebuild"))
        _rebuild_and_compare(gs, scene, p2, (nt, "moved"), again=False)
    finally:
        gs.release()


# ---------------------------------------------------------------------------------------------- B2: float classes

def _depth(dev, scene, gs):
    from rsd.frame import Renderer
    r = Renderer(scene, _cfg(), dev=dev, gpu_scene=gs)
    r.gbuffer()
    r.torch.cuda.synchronize()
    return r.depth.cpu().numpy()


@pytest.mark.parametrize("cls", E.FLOAT_CLASSES)
@pytest.mark.parametrize("base", E.FLOAT_BASES)
def test_float_classes_refit_rebuild_and_return(gpu, base, cls):
    """Ordinary upload -> update_positions(p) (host refit's bytes) -> rebuild_bvh() (host LBVH at p) ->
    update_positions(p0) (host refit of the rebuilt tree).  Where every position is finite the 75 x 45 G-buffer depth
    of the rebuilt scene equals that of a fresh static upload at p; infinite and NaN scenes are not rendered."""
    from rsd.frame import GpuScene, host_bvh, host_bvh_refit
    scene, p = E.float_class(base, cls)
    p0 = scene.positions
    built, off = host_bvh(scene)
    gs = GpuScene(gpu, scene, dynamic=True)
    fresh = None
    try:
        gs.update_positions(p)
        _same(gs.export_bvh()[0], host_bvh_refit(built, off, scene.indices, p), (base, cls, "refit"))
        tree, toff = _rebuild_and_compare(gs, scene, p, (base, cls), again=False)
        if cls in E.FINITE_CLASSES:
            at_p = dataclasses.replace(scene, positions=p)
            fresh = GpuScene(gpu, at_p)
            a, b = _depth(gpu, at_p, gs), _depth(gpu, at_p, fresh)
            assert a.shape == b.shape == (H, W) and a.tobytes() == b.tobytes(), (base, cls, "depth")
        gs.update_positions(p0)
        _same(gs.export_bvh()[0], host_bvh_refit(tree, toff, scene.indices, p0), (base, cls, "back on the rebuilt tree"))
        assert gs.dynamic_info().updates == 2
    finally:
        gs.release()
        if fresh is not None:
            fresh.release()


def test_a_referenced_nan(gpu):
    """One NaN coordinate of a vertex a triangle names: refit and rebuild leave the host refit's and the host builder's
    bytes.  The shared headers define where a NaN sorts (csrc/bvh_refit.h: by its integer key, a positive NaN above
    +inf) and that its code is 0 (csrc/lbvh.h); the numpy checkers use float min / max, which propagate a NaN, and are
    no reference here -- tests/test_dynamic_edges.py only checks that rsd_bvh_refit accepts the host tree."""
    from rsd.frame import GpuScene, host_bvh, host_bvh_refit
    scene, p = E.referenced_nan()
    built, off = host_bvh(scene)
    gs = GpuScene(gpu, scene, dynamic=True)
    try:
        gs.update_positions(p)
        _same(gs.export_bvh()[0], host_bvh_refit(built, off, scene.indices, p), "NaN: refit")
        tree, toff = _rebuild_and_compare(gs, scene, p, "NaN")
        gs.update_positions(scene.positions)
        _same(gs.export_bvh()[0], host_bvh_refit(tree, toff, scene.indices, scene.positions), "NaN: back")
    finally:
        gs.release()


# ---------------------------------------------------------------------------------------------- C: update_subset

def _subset_cases():
    nv = E.SUBSET_NX * E.SUBSET_NY
    rng = np.random.default_rng(77)
    cases = {}
    for count in (0, 1, 255, 256, 257, nv):
        cases[f"ascending-{count}"] = np.sort(rng.choice(nv, count, replace=False))
    cases["descending-257"] = np.sort(rng.choice(nv, 257, replace=False))[::-1]
    cases["descending-all"] = np.arange(nv)[::-1]
    cases["shuffled-256"] = rng.choice(nv, 256, replace=False)
    cases["shuffled-all"] = rng.permutation(nv)
    cases["duplicates-257"] = rng.choice(40, 257, replace=True) + 100  # every id several times, same position each
    ids = rng.choice(nv, 255, replace=False)
    mixed = np.concatenate([ids, [nv, nv + 1, nv, nv + 1]])  # 259 ids: the invalid ones in both blocks' lanes
    cases["out-of-range-259"] = mixed[rng.permutation(mixed.size)]
    cases["out-of-range-only"] = np.array([nv, nv + 1])
    return {k: np.ascontiguousarray(v, np.uint32) for k, v in cases.items()}


SUBSET_CASES = _subset_cases()


@pytest.fixture(scope="module")
def subset_scene():
    from rsd.frame import host_bvh
    scene = E.subset_grid()
    return (scene,) + host_bvh(scene)


@pytest.mark.parametrize("case", list(SUBSET_CASES))
def test_update_subset_at_its_contracts_edges(gpu, subset_scene, case):
    """The named valid vertices move, nothing else does: the tree is rsd_bvh_refit's at the expected positions and
    every vertex reads back bit for bit (all are named by triangles), the ones not named with their upload bits.
    include/rsd.h: an id >= vertex_count moves nothing -- refit_scatter_kernel's guard; ids vertex_count and
    vertex_count + 1 would otherwise land in the refit's parent words of nodes 0 .. 5 (inside the allocation)."""
    from rsd.frame import GpuScene, host_bvh_refit
    scene, built, off = subset_scene
    nv = scene.positions.shape[0]
    ids = SUBSET_CASES[case]
    rng = np.random.default_rng(ids.size + 5)
    target = np.ascontiguousarray(scene.positions + rng.uniform(-0.4, 0.4, scene.positions.shape).astype(np.float32))
    valid = ids < nv
    src = rng.uniform(-50.0, 50.0, (ids.size, 3)).astype(np.float32)  # arbitrary positions for the invalid ids
    src[valid] = target[ids[valid]]                                  # a repeated id repeats its position
    want = scene.positions.copy()
    want[ids[valid]] = target[ids[valid]]
    if case.startswith("out-of-range"):
        assert (~valid).sum() >= 2 and set(ids[~valid]) == {nv, nv + 1}
    if case.startswith("duplicates"):
        assert np.unique(ids).size < ids.size // 4
    gs = GpuScene(gpu, scene, dynamic=True)
    try:
        gs.update_subset(ids, src)
        have, hoff = gs.export_bvh()
        assert hoff == off
        if ids.size == 0 or not valid.any():
            _same(have, built, (case, "nothing moves: the upload's bytes"))
        _same(have, host_bvh_refit(built, off, scene.indices, want), case)
        got = morph_checker.export_positions(gs, scene.indices)
        assert _u32(got).tobytes() == _u32(want).tobytes(), (case, "positions")
        still = np.ones(nv, bool)
        still[ids[valid]] = False
        assert _u32(got[still]).tobytes() == _u32(scene.positions[still]).tobytes(), (case, "a vertex not named moved")
        assert gs.dynamic_info().updates == 1
        # a second call on the same object: back to the upload's positions through all ids
        gs.update_subset(np.arange(nv, dtype=np.uint32), scene.positions)
        _same(gs.export_bvh()[0], built, (case, "back"))
        assert gs.dynamic_info().updates == 2
    finally:
        gs.release()


# ---------------------------------------------------------------------------------------------- E: motion snapshot

@pytest.fixture(scope="module")
def mv(oracle, tmp_path_factory):
    import torch
    from rsd import abi
    return types.SimpleNamespace(torch=torch, abi=abi, L=abi.lib(), O=oracle,
                                 lib=MV.build(oracle, tmp_path_factory.mktemp("mvec_ref")))


@pytest.mark.parametrize("nv", E.SNAPSHOT_NV)
def test_motion_snapshot_at_every_tail(gpu, mv, nv):
    """track motion, update to P1, begin_frame, update to P2, rsd_gbuffer_motion: the motion vectors are the checker's
    for P1 -> P2, bit for bit (tests/test_gpu_mvec.py's rule).  3 * nv mod 4 is 0, 3, 2, 1: the last vertex lies in
    motion_snapshot_kernel's dword tail and owns pixels (tests/test_dynamic_edges.py); 1027 vertices take more than one
    block of vector lanes."""
    from rsd.frame import GpuScene
    scene = E.snapshot_grid(nv)
    p1, p2 = E.snapshot_motion(scene)
    size, cull = MV.SIZES[0], 0
    cam = MV.camera(scene, size)
    t, (w, h) = mv.torch, size
    gs = GpuScene(gpu, scene, dynamic=True, motion=True)
    try:
        gs.update_positions(p1)
        gs.begin_frame()
        gs.update_positions(p2)
        assert gs.motion_info().snapshots == 1
        out = {"depth": canary(t, (h, w), t.float32), "normal": canary(t, (h, w, 4), t.float32),
               "mvec": canary(t, (h, w, 2), t.float32), "mvecW": canary(t, (h, w, 4), t.float32)}
        p = lambda x: C.c_void_p(x.view.data_ptr())  # noqa: E731
        mv.abi.check(mv.L.rsd_gbuffer_motion(gs.h, C.byref(cam), C.byref(cam), w, h, cull, p(out["depth"]),
                                             p(out["normal"]), None, p(out["mvec"]), p(out["mvecW"]), None),
                     "rsd_gbuffer_motion")
        assert_canaries_intact(t, out, f"rsd_gbuffer_motion {nv}")
        got = {k: o.numpy() for k, o in out.items()}
        want = MV.run(mv.O, mv.lib, scene, p2, p1, cam, cam, size, cull)
        for key, ref in (("mvec", "mvec"), ("mvecW", "mvec_w")):
            bad = np.argwhere(MV.bits(got[key]) != MV.bits(want[ref]))
            assert bad.size == 0, (nv, key, len(bad), bad[:4].tolist())
        hit = want["prim"] != MV.MISS
        assert hit.any() and MV.bits(got["mvec"])[hit].any()
    finally:
        t.cuda.synchronize()
        gs.release()
