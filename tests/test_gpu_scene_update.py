"""GPU: dynamic scenes (rsd_scene_upload_dynamic, rsd_scene_update_positions / _subset, rsd_scene_rebuild_entry_grid).

Three statements, all bitwise:
  * after an update the device BVH is rsd_bvh_refit's bytes (pinned to an independent recomputation by
    tests/test_bvh_refit.py) -- from a host pointer, a device pointer and a subset update, along P0 -> P1 -> P2 -> P0
    on one scene object (the arrival counters reset themselves), on the small shapes and on a ~50 k-triangle scene whose
    refit spans many workgroups and CUs;
  * everything rendered from the refitted scene equals what a FRESH upload of the moved scene renders (the canonical
    any-hit stream does not depend on the tree) and what the CPU oracle computes from the moved positions; the
    traversal-order and wavefront streams, tree-dependent by definition, equal the oracle walking the exported
    refitted tree;
  * the stale entry grid is dropped, not used, until it is rebuilt.

Frames are 75 x 45 (8 x 8 tiles partial on both axes), exact numerics.  The motions are random per-vertex jitter plus
a translated part, which leaves no exact equal-t ties between different surfaces, so the G-buffer's normals are compared
as well as its depth."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import scenes_adversarial
from helpers import oracle_frame, to_oracle

pytestmark = pytest.mark.gpu

W, H = 75, 45


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


def _moved(scene, seed, part=(0.4, 0.3, -0.5)):
    """Per-vertex jitter of a fixed seed plus the last eighth of the triangles translated by `part`."""
    rng = np.random.default_rng(seed)
    p = scene.positions + (0.02 * rng.standard_normal(scene.positions.shape)).astype(np.float32)
    v = np.unique(scene.indices[-max(1, scene.indices.shape[0] // 8):])
    p[v] += np.float32(part)
    return np.ascontiguousarray(p, np.float32)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rsd.frame import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def small():
    from rsd.scenes import make_scene
    return make_scene("arcade_tiny", target_tris=3000)


def _shape_scene(name):
    from rsd.ingest import load_obj
    from rsd.scenes import Scene, make_scene
    from conftest import ROOT
    cam = dict(pos=[0.0, 0.0, 3.0], target=[0.0, 0.0, 0.0], up=[0.0, 1.0, 0.0])
    if name == "one_triangle":
        return Scene(name, np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], np.float32), np.array([[0, 1, 2]], np.uint32),
                     np.zeros(1, np.uint32), cam)
    if name == "grid_24":
        p = np.array([[x, y, 0.25 * x * y] for y in range(4) for x in range(5)], np.float32)
        i = np.arange(20).reshape(4, 5)
        a, b, c, d = i[:-1, :-1], i[:-1, 1:], i[1:, 1:], i[1:, :-1]
        t = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 2).reshape(-1, 3).astype(np.uint32)
        return Scene(name, p, np.ascontiguousarray(t), np.zeros(24, np.uint32), cam)
    if name == "slivers":
        return scenes_adversarial.make("slivers")
    if name == "crate":
        return load_obj(ROOT / "tests" / "fixtures" / "crate.obj").build("crate")
    if name == "arcade_3000":
        return make_scene("arcade_tiny", target_tris=3000)
    if name == "arcade_50k":  # thousands of wide nodes: the refit's climb crosses workgroups, CUs and XCDs
        return make_scene("arcade_tiny", target_tris=50_000)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["one_triangle", "grid_24", "slivers", "crate", "arcade_3000", "arcade_50k"])
def test_updates_leave_the_host_refit_bytes(gpu, name):
    """P0 -> P1 (host pointer) -> P2 (device pointer) -> P1 again (subset update of the vertices that differ) -> P0:
    after each step the exported BVH is rsd_bvh_refit of the upload's bytes, and at the end the upload's bytes."""
    import torch
    from rsd.frame import GpuScene, host_bvh, host_bvh_refit
    scene = _shape_scene(name)
    if name == "arcade_50k":
        assert scene.indices.shape[0] > 40_000
    p0, p1, p2 = scene.positions, _moved(scene, 1), _moved(scene, 2, part=(-30.0, 500.0, 2.0))
    built, off = host_bvh(scene)
    gs = GpuScene(gpu, scene, dynamic=True)
    try:
        got, goff = gs.export_bvh()
        assert goff == off and np.array_equal(_u32(got), _u32(built)), "a dynamic upload holds rsd_bvh_build's bytes"
        info = gs.dynamic_info()
        assert info.dynamic == 1 and info.updates == 0 and info.entry_grid_current == 1 and info.dynamic_bytes > 0

        def check(p, what):
            want = host_bvh_refit(built, off, scene.indices, p)
            have, _ = gs.export_bvh()
            bad = np.flatnonzero(_u32(have) != _u32(want))
            assert bad.size == 0, (name, what, bad.size, bad[:8])

        gs.update_positions(p1)
        check(p1, "host pointer")
        gs.update_positions(torch.from_numpy(p2).cuda())
        check(p2, "device pointer")
        ids = np.flatnonzero((p1 != p2).any(axis=1)).astype(np.uint32)
        assert 0 < ids.size
        gs.update_subset(ids, p1[ids])
        check(p1, "subset")
        gs.update_positions(p0)
        have, _ = gs.export_bvh()
        assert np.array_equal(_u32(have), _u32(built)), "back at P0: the upload's bytes"
        assert gs.dynamic_info().updates == 4
    finally:
        gs.release()


def _depth_peel(r, depth, sep=0.5):
    from rsd import abi
    out = r.torch.full((H, W), -7.0, dtype=r.torch.float32, device=depth.device)
    abi.check(abi.lib().rsd_depth_peel(r.gscene.h, C.byref(r.cam), W, H, r.cfg.cull_mode, C.c_void_p(depth.data_ptr()),
                                       float(sep), 1, C.c_void_p(out.data_ptr()), r.stream), "rsd_depth_peel")
    return out


def _render(dev, scene, gs):
    """Every scene-reading entry on `gs` (scene: the host Scene with the positions gs now holds)."""
    from rsd import abi
    from rsd.frame import Renderer
    out = {}
    r = Renderer(scene, _cfg(), dev=dev, gpu_scene=gs)
    r.gbuffer()
    out["depth"], out["normals"] = r.depth.clone(), r.normals.clone()
    out["peel"] = _depth_peel(r, r.depth)
    amb, dist = r.rtao(spp=2, frame_index=3)
    out["rtao"], out["rtao_t"] = amb, dist
    for N in (4, 8):
        for interval in (True, False):
            q = Renderer(scene, _cfg(sd_samples=N, ray_interval=interval), dev=dev, gpu_scene=gs)
            q.gbuffer()
            q.clear_intervals()
            q.pass1()
            q.sd.zero_()
            q.sd_trace()
            out[f"sd_N{N}_iv{int(interval)}"] = q.sd.clone()
    # the raster map keeps fragments behind the first layer: no culling and a wide AO radius give it some to keep
    q = Renderer(scene, _cfg(sd_guard_px=0, jitter=False, cull_mode=abi.CULL_NONE, radius=6.0), dev=dev, gpu_scene=gs)
    q.gbuffer()
    q.clear_intervals()
    q.pass1()
    q.sd.zero_()
    q.sd_raster()
    out["sd_raster"] = q.sd.clone()
    for mode, key in ((abi.DEPTH_STOCHASTIC, "ao_sd"), (abi.DEPTH_RAYTRACED, "ao_rt")):
        q = Renderer(scene, _cfg(secondary=mode), dev=dev, gpu_scene=gs)
        q.gbuffer()
        q.frame()
        out[key] = q.ao.clone()
        if mode == abi.DEPTH_STOCHASTIC:
            out["frame"] = q.numpy()
            out["frame_r"] = q
    r.torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}


@pytest.fixture(scope="module")
def parity(gpu, small):
    """The small scene moved to P1 three ways: refitted (after a detour through P2), uploaded fresh, and left alone."""
    from rsd.frame import GpuScene
    p1 = _moved(small, 1)
    moved = dataclasses.replace(small, positions=p1)
    dyn = GpuScene(gpu, small, dynamic=True)
    dyn.update_positions(_moved(small, 2))
    dyn.update_positions(p1)
    fresh = GpuScene(gpu, moved)
    static = GpuScene(gpu, small)
    out = dict(refit=_render(gpu, moved, dyn), fresh=_render(gpu, moved, fresh), old=_render(gpu, small, static),
               moved=moved, dyn=dyn)
    yield out
    for s in (dyn, fresh, static):
        s.release()


KEYS = ["depth", "normals", "peel", "rtao", "rtao_t", "sd_N4_iv1", "sd_N4_iv0", "sd_N8_iv1", "sd_N8_iv0", "sd_raster",
        "ao_sd", "ao_rt"]


@pytest.mark.parametrize("key", KEYS)
def test_refitted_scene_renders_like_a_fresh_upload(parity, key):
    a, b = parity["refit"][key], parity["fresh"][key]
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), key
    if key in ("depth", "sd_N4_iv1", "sd_N8_iv0", "sd_raster", "ao_sd", "ao_rt", "rtao"):
        assert a.tobytes() != parity["old"][key].tobytes(), "the motion does not show in this output"


def test_refitted_scene_matches_the_oracle(oracle, parity):
    """The whole StochasticDepth frame -- G-buffer, intervals, SD map, AO -- of the CPU oracle given the moved positions."""
    O, g, r, moved = oracle, parity["refit"]["frame"], parity["refit"]["frame_r"], parity["moved"]
    osc = O.Scene(moved.positions, moved.indices, moved.flags)
    o = oracle_frame(O, osc, to_oracle(r.cam, O.Camera), to_oracle(r.vao, O.VAOData), to_oracle(r.sdp, O.SDParams),
                     to_oracle(r.svp, O.SVAOParams), W, H, r.sd_w, r.sd_h)
    assert o["stats"][0] > 100, "hardly any live SD ray: the frame is degenerate"
    assert np.array_equal(_u32(g["depth"]), _u32(o["depth"]))
    assert np.array_equal(g["ray_min"], o["ray_min"]) and np.array_equal(g["ray_max"], o["ray_max"])
    assert np.array_equal(_u32(g["sd"]), _u32(o["sd"]))
    assert np.array_equal(g["ao"], o["ao"])


@pytest.mark.parametrize("order", [1, 2])
def test_tree_dependent_streams_walk_the_refitted_tree(oracle, gpu, parity, order):
    """RSD_HIT_ORDER_TRAVERSAL / _WAVEFRONT against the oracle walking the exported refitted tree."""
    from rsd.frame import Renderer
    moved, dyn = parity["moved"], parity["dyn"]
    r = Renderer(moved, _cfg(hit_order=order), dev=gpu, gpu_scene=dyn)
    r.gbuffer()
    r.clear_intervals()
    r.pass1()
    r.sd.zero_()
    r.sd_trace()
    g = r.numpy()
    bvh, off = dyn.export_bvh()
    osc = oracle.Scene(moved.positions, moved.indices, moved.flags)
    cam, sdp = to_oracle(r.cam, oracle.Camera), to_oracle(r.sdp, oracle.SDParams)
    args = (cam, sdp, g["depth"], g["ray_min"], g["ray_max"], r.sd_w, r.sd_h)
    if order == 2:
        soft = min(208 - 3 * int(dyn.info.wide_depth), 160)
        sd, stats = oracle.sd_trace_wavefront(osc, bvh, off, soft, *args)
    else:
        sd, stats = oracle.sd_trace_ordered(osc, bvh, off, *args)
    assert stats[0] > 100
    assert np.array_equal(_u32(g["sd"]), _u32(sd))


def test_stale_entry_grid_is_dropped_until_rebuilt(oracle, gpu, small, monkeypatch):
    """The last eighth of the triangles rises 3 m into air that was empty at upload: the frontiers of the cells there
    cannot cover them.  The SD map right after the update is the oracle's (it would miss them through the stale grid),
    the info says stale; after the rebuild it says current, an instrumented trace looks cells up, same map."""
    from rsd.frame import GpuScene, Renderer
    monkeypatch.delenv("RSD_TRACE_ENTRY", raising=False)
    monkeypatch.delenv("RSD_TRACE_WALK", raising=False)
    p1 = _moved(small, 5, part=(0.0, 3.0, 0.0))
    moved = dataclasses.replace(small, positions=p1)
    gs = GpuScene(gpu, small, dynamic=True)
    try:
        assert gs.info.entry_cells > 0
        r = Renderer(small, _cfg(), dev=gpu, gpu_scene=gs)

        def trace(counters=False):
            r.gbuffer()
            r.clear_intervals()
            r.pass1()
            r.sd.zero_()
            cnt = r.sd_trace(counters=counters)
            return r.numpy(), cnt

        before, cnt = trace(counters=True)
        assert cnt.entry_lookups > 0, "the fresh scene's trace uses its grid"
        r.update_positions(p1)
        assert np.array_equal(r.scene.positions, p1) and np.array_equal(small.positions, _shape_scene("arcade_3000").positions)
        info = gs.dynamic_info()
        assert info.entry_grid_current == 0 and info.updates == 1
        after, cnt = trace(counters=True)
        assert cnt.entry_lookups == 0, "a stale grid is dropped: the walks start at the root"
        osc = oracle.Scene(p1, moved.indices, moved.flags)
        sd, stats = oracle.sd_trace(osc, to_oracle(r.cam, oracle.Camera), to_oracle(r.sdp, oracle.SDParams),
                                    after["depth"], after["ray_min"], after["ray_max"], r.sd_w, r.sd_h)
        assert stats[0] > 100
        assert np.array_equal(_u32(after["sd"]), _u32(sd))
        assert not np.array_equal(_u32(after["sd"]), _u32(before["sd"]))
        gs.rebuild_entry_grid()
        info = gs.dynamic_info()
        assert info.entry_grid_current == 1 and gs.info.entry_cells > 0
        again, cnt = trace(counters=True)
        assert cnt.entry_lookups > 0
        assert np.array_equal(_u32(again["sd"]), _u32(after["sd"]))
        plain, _ = trace()
        assert np.array_equal(_u32(plain["sd"]), _u32(after["sd"]))
    finally:
        gs.release()


def test_a_static_scene_refuses_updates(gpu, small):
    import torch
    from rsd import abi
    from rsd.frame import GpuScene, Renderer
    gs = GpuScene(gpu, small)
    try:
        r = Renderer(small, _cfg(), dev=gpu, gpu_scene=gs)
        r.gbuffer()
        before, bvh = r.numpy()["depth"], gs.export_bvh()[0]
        info = gs.dynamic_info()
        assert info.dynamic == 0 and info.dynamic_bytes == 0 and info.entry_grid_current == 1
        with pytest.raises(abi.RsdError, match="not dynamic") as e:
            gs.update_positions(_moved(small, 1))
        assert e.value.status == abi.ERR_INVALID_ARG
        with pytest.raises(abi.RsdError, match="not dynamic"):
            gs.update_subset(np.zeros(1, np.uint32), np.zeros((1, 3), np.float32))
        torch.cuda.synchronize()
        r.gbuffer()
        assert np.array_equal(_u32(r.numpy()["depth"]), _u32(before))
        assert np.array_equal(_u32(gs.export_bvh()[0]), _u32(bvh))
    finally:
        gs.release()


def test_wrong_vertex_count_is_refused(gpu, small):
    from rsd import abi
    from rsd.frame import GpuScene
    gs = GpuScene(gpu, small, dynamic=True)
    try:
        with pytest.raises(abi.RsdError, match="vertex_count") as e:
            gs.update_positions(small.positions[:-1])
        assert e.value.status == abi.ERR_INVALID_ARG and gs.dynamic_info().updates == 0
    finally:
        gs.release()
