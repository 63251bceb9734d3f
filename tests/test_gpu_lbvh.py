"""GPU: rsd_scene_rebuild_bvh (csrc/lbvh.hip) -- a dynamic scene's tree rebuilt on the device, in place.

All statements are bitwise:
  * after rebuild_bvh() the exported BVH is rsd_bvh_build_lbvh of the current positions (pinned to an independent
    restatement by tests/test_lbvh.py) -- at the upload's positions, after a large motion, and unchanged by a second
    rebuild; a later update leaves rsd_bvh_refit's bytes of the rebuilt tree;
  * everything tests/test_gpu_scene_update.py renders equals a fresh upload of the moved scene, and the oracle's frame;
    the tree-dependent streams equal the oracle walking the exported rebuilt tree;
  * the entry grid is stale after a rebuild and changes nothing once rebuilt;
  * rig, morph table and motion tracking survive: animate(t) after a rebuild gives the positions, the frame and the
    motion vectors it gives without one.
Every input is a valid scene; frames are test_gpu_scene_update.py's 75 x 45."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import lbvh_scenes
import morph_checker
from helpers import oracle_frame, to_oracle
from test_gpu_scene_update import H, KEYS, W, _cfg, _render, _u32

pytestmark = pytest.mark.gpu


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
    return lbvh_scenes.scene("arcade_3000")


def _same(have, want, what):
    bad = np.flatnonzero(_u32(have) != _u32(want))
    assert have.nbytes == want.nbytes and bad.size == 0, (what, have.nbytes, want.nbytes, bad.size, bad[:8])


@pytest.mark.parametrize("name", lbvh_scenes.SCENES)
def test_rebuild_leaves_the_host_builders_bytes(gpu, name):
    """Rebuild at the upload's positions, again (nothing changes), after a large motion, and an update after that."""
    from rsd.frame import GpuScene, host_bvh_lbvh, host_bvh_refit
    scene = lbvh_scenes.scene(name)
    nt = scene.indices.shape[0]
    p1, p2 = lbvh_scenes.large_motion(scene), lbvh_scenes.moved(scene, 2)
    gs = GpuScene(gpu, scene, dynamic=True)
    try:
        assert gs.rebuild_info().rebuilds == 0 and gs.rebuild_info().device_ms == 0.0
        want, woff = host_bvh_lbvh(scene)
        gs.rebuild_bvh()
        have, off = gs.export_bvh()
        assert off == woff
        _same(have, want, (name, "upload positions"))
        info, dyn = gs.rebuild_info(), gs.dynamic_info()
        assert (info.rebuilds, info.node_count) == (1, off // 8) and info.wide_depth == gs.info.wide_depth >= 1
        assert info.device_ms > 0.0 and gs.info.node_count == off // 8 and gs.info.triangle_count == nt
        assert info.wide_depth <= (30 + max(0, nt - 1).bit_length()) // 2 + 1
        assert dyn.dynamic == 1 and dyn.updates == 0 and dyn.entry_grid_current == (0 if gs.info.entry_cells else 1)
        gs.rebuild_bvh()
        again, off2 = gs.export_bvh()
        assert off2 == off and gs.rebuild_info().rebuilds == 2
        _same(again, want, (name, "second rebuild"))
        # a large motion: the refit keeps the topology, the rebuild follows the geometry
        gs.update_positions(p1)
        _same(gs.export_bvh()[0], host_bvh_refit(want, woff, scene.indices, p1), (name, "update after a rebuild"))
        gs.rebuild_bvh()
        want1, woff1 = host_bvh_lbvh(dataclasses.replace(scene, positions=p1))
        have1, off1 = gs.export_bvh()
        assert off1 == woff1
        _same(have1, want1, (name, "large motion"))
        gs.update_positions(p2)
        _same(gs.export_bvh()[0], host_bvh_refit(want1, woff1, scene.indices, p2), (name, "update after the second tree"))
        assert gs.dynamic_info().updates == 2 and gs.rebuild_info().rebuilds == 3
    finally:
        gs.release()


@pytest.fixture(scope="module")
def parity(gpu, small):
    """The small scene moved far three ways: refitted then rebuilt, uploaded fresh, and left alone."""
    from rsd.frame import GpuScene
    p1 = lbvh_scenes.moved(small, 1)
    moved = dataclasses.replace(small, positions=p1)
    dyn = GpuScene(gpu, small, dynamic=True)
    dyn.update_positions(lbvh_scenes.large_motion(small))
    dyn.rebuild_bvh()
    dyn.update_positions(p1)
    dyn.rebuild_bvh()
    fresh = GpuScene(gpu, moved)
    static = GpuScene(gpu, small)
    out = dict(rebuilt=_render(gpu, moved, dyn), fresh=_render(gpu, moved, fresh), old=_render(gpu, small, static),
               moved=moved, dyn=dyn)
    yield out
    for s in (dyn, fresh, static):
        s.release()


@pytest.mark.parametrize("key", KEYS)
def test_rebuilt_scene_renders_like_a_fresh_upload(parity, key):
    a, b = parity["rebuilt"][key], parity["fresh"][key]
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), key
    if key in ("depth", "sd_N4_iv1", "sd_N8_iv0", "sd_raster", "ao_sd", "ao_rt", "rtao"):
        assert a.tobytes() != parity["old"][key].tobytes(), "the motion does not show in this output"


def test_rebuilt_scene_matches_the_oracle(oracle, parity):
    O, g, r, moved = oracle, parity["rebuilt"]["frame"], parity["rebuilt"]["frame_r"], parity["moved"]
    osc = O.Scene(moved.positions, moved.indices, moved.flags)
    o = oracle_frame(O, osc, to_oracle(r.cam, O.Camera), to_oracle(r.vao, O.VAOData), to_oracle(r.sdp, O.SDParams),
                     to_oracle(r.svp, O.SVAOParams), W, H, r.sd_w, r.sd_h)
    assert o["stats"][0] > 100, "hardly any live SD ray: the frame is degenerate"
    assert np.array_equal(_u32(g["depth"]), _u32(o["depth"]))
    assert np.array_equal(g["ray_min"], o["ray_min"]) and np.array_equal(g["ray_max"], o["ray_max"])
    assert np.array_equal(_u32(g["sd"]), _u32(o["sd"]))
    assert np.array_equal(g["ao"], o["ao"])


@pytest.mark.parametrize("order", [1, 2])
def test_tree_dependent_streams_walk_the_rebuilt_tree(oracle, gpu, parity, order):
    """RSD_HIT_ORDER_TRAVERSAL / _WAVEFRONT against the oracle walking the exported rebuilt tree."""
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
        soft = min(208 - 3 * int(dyn.rebuild_info().wide_depth), 160)
        sd, stats = oracle.sd_trace_wavefront(osc, bvh, off, soft, *args)
    else:
        sd, stats = oracle.sd_trace_ordered(osc, bvh, off, *args)
    assert stats[0] > 100
    assert np.array_equal(_u32(g["sd"]), _u32(sd))


def test_entry_grid_is_stale_after_a_rebuild_and_harmless_once_rebuilt(gpu, small, monkeypatch):
    from rsd.frame import GpuScene, Renderer
    monkeypatch.delenv("RSD_TRACE_ENTRY", raising=False)
    monkeypatch.delenv("RSD_TRACE_WALK", raising=False)
    gs = GpuScene(gpu, small, dynamic=True)
    try:
        assert gs.info.entry_cells > 0 and gs.dynamic_info().entry_grid_current == 1
        r = Renderer(small, _cfg(), dev=gpu, gpu_scene=gs)

        def trace():
            r.gbuffer()
            r.clear_intervals()
            r.pass1()
            r.sd.zero_()
            cnt = r.sd_trace(counters=True)
            return r.numpy()["sd"], cnt

        before, cnt = trace()
        assert cnt.entry_lookups > 0
        gs.rebuild_bvh()
        assert gs.dynamic_info().entry_grid_current == 0
        stale, cnt = trace()
        assert cnt.entry_lookups == 0, "the old tree's grid is dropped: its items name nodes that no longer exist"
        assert np.array_equal(_u32(stale), _u32(before)), "the canonical map does not depend on the tree"
        gs.rebuild_entry_grid()
        assert gs.dynamic_info().entry_grid_current == 1 and gs.info.entry_cells > 0
        current, cnt = trace()
        assert cnt.entry_lookups > 0
        assert np.array_equal(_u32(current), _u32(before))
    finally:
        gs.release()


def test_rig_morph_and_motion_survive_a_rebuild(gpu, tmp_path):
    """The glTF cylinder (skin, two morph targets, motion tracked): pose, snapshot, rebuild, pose again -- positions,
    frame and motion vectors equal those of the same calls without the rebuild."""
    import torch
    import gltf_scenes
    from rsd import abi
    from rsd.frame import GpuScene, Renderer, look_at
    from rsd.gltf import load_gltf
    from test_gpu_gltf import _cfg as gltf_cfg
    w, _ = gltf_scenes.cylinder()
    scene = load_gltf(w.save(tmp_path / "cylinder.glb", "glb"))
    cam = look_at(scene.camera["pos"], scene.camera["target"], scene.camera["up"], gltf_cfg())
    out = []
    for rebuild in (False, True):
        gs = GpuScene(gpu, scene, dynamic=True, motion=True)
        try:
            gs.animate(0.5)
            gs.begin_frame()
            if rebuild:
                gs.rebuild_bvh()
                assert gs.rebuild_info().rebuilds == 1
            gs.animate(1.0)
            rig, morph, motion = gs.rig_info(), gs.morph_info(), gs.motion_info()
            assert (rig.attached, rig.count, morph.attached, morph.entry_count) == (1, 16, 1, 15)
            assert motion.tracked == 1 and motion.snapshots == 1 and gs.dynamic_info().updates == 2
            z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")  # noqa: E731
            depth, normal, pos_w, mvec = z(H, W), z(H, W, 4), z(H, W, 4), z(H, W, 2)
            p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
            abi.check(abi.lib().rsd_gbuffer_motion(gs.h, C.byref(cam), C.byref(cam), W, H, 0, p(depth), p(normal),
                                                   p(pos_w), p(mvec), None, None), "rsd_gbuffer_motion")
            r = Renderer(scene, gltf_cfg(), dev=gpu, gpu_scene=gs)
            r.gbuffer()
            r.frame()
            torch.cuda.synchronize()
            f = r.numpy()
            out.append(dict(positions=morph_checker.export_positions(gs, scene.indices), mvec=mvec.cpu().numpy(),
                            depth=depth.cpu().numpy(), sd=f["sd"], ao=f["ao"], z=f["depth"]))
        finally:
            gs.release()
    assert np.abs(out[0]["mvec"]).max() > 1e-3 and (out[0]["sd"] != 0).any(), "the frame is degenerate"
    for key in out[0]:
        assert out[0][key].shape == out[1][key].shape and out[0][key].tobytes() == out[1][key].tobytes(), key


def test_render_graph_rebuild(gpu, small):
    """RenderGraph.rebuild_bvh between executes: the graph's AO does not change, the scene counts the rebuild."""
    import torch
    from conftest import ROOT
    from helpers import small_frame_config
    from rsd import graph as rg
    from rsd.frame import GpuScene, make_camera
    cfg = small_frame_config()
    gs = GpuScene(gpu, small, dynamic=True)
    g = rg.load_script(ROOT / "tests" / "graphs" / "svao_temporal.py")["SVAOTemporal"]
    try:
        g.mark_output("GBufferRaster.posW")
        g.set_scene(gs.h, make_camera(small, cfg))
        g.compile(cfg.fb_w, cfg.fb_h)
        g.execute()
        before = g.output_tensor("GBufferRaster.posW").cpu().numpy()
        g.rebuild_bvh()
        assert gs.rebuild_info().rebuilds == 1
        g.execute()
        after = g.output_tensor("GBufferRaster.posW").cpu().numpy()
        assert before.tobytes() == after.tobytes() and np.abs(before).max() > 0
    finally:
        torch.cuda.synchronize()
        g.close()
        gs.release()


def test_a_static_scene_refuses_a_rebuild(gpu, small):
    from rsd import abi
    from rsd.frame import GpuScene
    gs = GpuScene(gpu, small)
    try:
        bvh = gs.export_bvh()[0]
        with pytest.raises(abi.RsdError, match="not dynamic") as e:
            gs.rebuild_bvh()
        assert e.value.status == abi.ERR_INVALID_ARG
        info = gs.rebuild_info()
        assert info.rebuilds == 0 and info.node_count == gs.info.node_count and info.device_ms == 0.0
        assert np.array_equal(_u32(gs.export_bvh()[0]), _u32(bvh))
    finally:
        gs.release()
