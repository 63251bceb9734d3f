"""GPU: the state an SD trace leaves behind for the next one.  rsd_sd_trace* keeps an SdWorkspace per (scene, stream)
(csrc/rsd_internal.h): the double-buffered queue control that call k zeroes for call k + 1, the grow-only live-ray
workspace whose sections sd_plan lays out anew for every call's sizes, the cached ray table, the raster walk's grow-only
scratch, and the list of workspaces, capped at 64 streams.  Every test here runs a sequence of different calls through
ONE workspace, forwards and in reverse, and asks of every call the raw bits of the oracle's map -- and of the same call
on a fresh scene that has traced nothing else, which tells a fault of the carried state from a fault of the walk.

The cases, their inputs (uploaded here: linear depth and interval maps from the oracle) and the oracle's maps are those
of tests/test_trace_state.py, which shows on the CPU that neighbouring cases have different maps.  Before every trace the
intervals are restored and the map is filled with a sentinel no result equals."""
import ctypes as C

import numpy as np
import pytest

import test_trace_state as TS
from helpers import SENTINEL, report, sentinel_array
from test_gpu_adversarial_walk import ENV

pytestmark = pytest.mark.gpu

# every knob a step may set: cleared before each trace (librsd reads them per call)
KNOBS = ("RSD_TRACE_WALK", "RSD_TRACE_HYBRID", "RSD_TRACE_HYBRID16", "RSD_TRACE_ENTRY", "RSD_TRACE_SPEC", "RSD_TRACE_LPT",
         "RSD_TRACE_POOL", "RSD_TRACE_PRIO", "RSD_TRACE_ROWPRIO", "RSD_TRACE_SPREAD", "RSD_TRACE_WAVES_PER_CU",
         "RSD_TRACE_HYBRID_ROWWPC", "RSD_TRACE_QRANGE", "RSD_SETUP_TWOPASS", "RSD_SETUP_DIAG")
WALK_ENV = dict(ENV, twopass=dict(RSD_SETUP_TWOPASS="on"))
ORDERS = ("forward", "reverse")


def ordered(steps, order):
    return list(steps) if order == "forward" else list(steps)[::-1]


class Gpu:
    """One rsd_device, one GpuScene per scene and one Renderer per case on top of it: every trace of a scene on a
    stream goes through the same workspace."""

    def __init__(self, oracle):
        import torch
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from rsd import abi
        from rsd.frame import Device
        self.torch, self.abi, self.oracle = torch, abi, oracle
        self.dev = Device(0)
        self.scenes, self.renderers, self.fresh_maps = {}, {}, {}

    def scene(self, name):
        if name not in self.scenes:
            from rsd.frame import GpuScene
            self.scenes[name] = GpuScene(self.dev, TS.host_scene(name))
        return self.scenes[name]

    def new_renderer(self, name, gscene=None):
        """A renderer of case `name` holding the case's camera, parameters and inputs."""
        from rsd.frame import Renderer
        t, b = self.torch, TS.built(self.oracle, name)
        r = Renderer(b.scene, b.cfg, dev=self.dev, gpu_scene=gscene or self.scene(b.case.scene))
        assert (r.sd_w, r.sd_h) == (b.sd_w, b.sd_h)
        r.cam = b.cam
        r.sdp = self.abi.SDParams.from_buffer_copy(b.sdp)
        r.depth.copy_(t.from_numpy(b.depth.copy()))
        r.saved = t.from_numpy(np.stack([b.rmin, b.rmax]).view(np.int32)).to(r.depth.device)
        r.built = b
        t.cuda.synchronize()
        return r

    def renderer(self, name):
        if name not in self.renderers:
            self.renderers[name] = self.new_renderer(name)
        return self.renderers[name]

    def env(self, monkeypatch, env):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)

    def prepare(self, r):
        """Restore the intervals (a trace may consume them) and fill the map with the sentinel."""
        r.ray_minmax.copy_(r.saved)
        r.sd.view(self.torch.uint8).fill_(SENTINEL)

    def trace(self, monkeypatch, r, env=None, **kw):
        """One prepared trace of r under the knobs `env`; returns (the map, the counters or None)."""
        self.env(monkeypatch, env or {})
        self.prepare(r)
        c = r.sd_trace(**kw)
        self.torch.cuda.synchronize()
        return r.sd.cpu().numpy(), c

    def fresh(self, monkeypatch, name, env=None):
        """The map of the same call on a fresh GpuScene that has traced nothing else (once per case and knob set)."""
        key = (name, tuple(sorted((env or {}).items())))
        if key not in self.fresh_maps:
            from rsd.frame import GpuScene
            gs = GpuScene(self.dev, TS.host_scene(TS.CASES[name].scene))
            try:
                self.fresh_maps[key] = self.trace(monkeypatch, self.new_renderer(name, gs), env)[0]
            finally:
                gs.release()
        return self.fresh_maps[key]

    def check(self, monkeypatch, name, got, what, env=None):
        """`got` carries the oracle's bits and those of the fresh scene's call."""
        want = TS.built(self.oracle, name).want
        fresh = self.fresh(monkeypatch, name, env)
        bad = (TS.bits(got) != TS.bits(want)).any(axis=(0, 3))
        bad_fresh = (TS.bits(fresh) != TS.bits(want)).any(axis=(0, 3))
        untouched = (TS.bits(got) == TS.bits(sentinel_array(got.shape, np.float32))).any(axis=(0, 3))
        assert not bad.any() and not bad_fresh.any(), (
            f"{what}: {int(bad.sum())} texels differ from the oracle on the shared workspace (first (y, x) "
            f"{np.argwhere(bad)[:4].tolist()}, {int(untouched.sum())} never written), {int(bad_fresh.sum())} on a fresh "
            "scene" + ("" if bad_fresh.any() else ": the state carried between calls"))

    def close(self):
        for s in self.scenes.values():
            s.release()
        self.dev.close()


@pytest.fixture(scope="module")
def gpu(oracle):
    g = Gpu(oracle)
    yield g
    g.close()


def run(gpu, monkeypatch, names, label, env=None, **kw):
    for i, name in enumerate(names):
        got, _ = gpu.trace(monkeypatch, gpu.renderer(name), env, **kw)
        gpu.check(monkeypatch, name, got, f"{label} step {i} ({name})", env)


# ---- sizes, N, MAX_COUNT

@pytest.mark.timeout(120)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seq", ["sizes", "samples", "max_count"])
def test_sizes_on_one_workspace(gpu, monkeypatch, seq, order):
    """BIG -> SMALL -> ODD -> BIG -> SMALL (the allocation grows once, then holds smaller calls whose sections lie
    elsewhere in it), N 16 -> 1 -> 4, MAX_COUNT 32 -> 4 -> 8."""
    run(gpu, monkeypatch, ordered(TS.SEQUENCES[seq], order), f"{seq} {order}")


# ---- walks

WALK_STEPS = ["raster", "fused", "split", "quad", "hybrid", "hybrid16", "twopass", "raster", "quad"]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("base", ["big", "layers"])
def test_walks_on_one_workspace(gpu, monkeypatch, base, order):
    """Every walk after every other on one workspace: each uses queue-control words of its own (the raster walk's
    live-tile count, the two-pass setup's touch counts, the hybrid's second heads, the short-ray counts).  The
    instrumented trace after each step names the walk the step's knobs select and writes the same bits."""
    abi = gpu.abi
    named = dict(raster=abi.WALK_RASTER, fused=abi.WALK_FUSED, split=abi.WALK_SPLIT, quad=abi.WALK_QUAD,
                 hybrid=abi.WALK_HYBRID, hybrid16=abi.WALK_HYBRID, twopass=abi.WALK_HYBRID)
    for i, walk in enumerate(ordered(WALK_STEPS, order)):
        name = base + "_n16" if walk == "hybrid16" else base
        what = f"walks {order} step {i} ({walk}, {name})"
        r = gpu.renderer(name)
        got, _ = gpu.trace(monkeypatch, r, WALK_ENV[walk])
        gpu.check(monkeypatch, name, got, what, WALK_ENV[walk])
        got, c = gpu.trace(monkeypatch, r, WALK_ENV[walk], counters=True)
        assert int(c.walk) == named[walk], (what, abi.WALK_NAMES[int(c.walk)])
        gpu.check(monkeypatch, name, got, what + ", instrumented", WALK_ENV[walk])


# ---- the ray table's key

@pytest.mark.timeout(120)
@pytest.mark.parametrize("order", ORDERS)
def test_ray_table_follows_every_term_of_its_key(gpu, monkeypatch, order):
    """One frame size; between consecutive traces exactly one of jitter, cam.jitterX, cam.jitterY, the guard band, the
    pose (a new W) and the camera's position (U, V, W kept) changes, last nothing (the cached table)."""
    names = ordered(TS.SEQUENCES["ray_table"], order)
    sizes = {(gpu.renderer(n).sd_w, gpu.renderer(n).sd_h) for n in names}
    assert len(sizes) == 1
    run(gpu, monkeypatch, names, f"ray table {order}")


# ---- instrumented between uninstrumented

@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", ["counters", "throughput"])
def test_instrumented_between_plain_traces(gpu, monkeypatch, kind):
    """Plain -> instrumented (the 256-entry pool, never the hybrid) -> plain at BIG; the same around a trace with
    RSD_SD_THROUGHPUT.  (The sequence is its own reverse.)"""
    r = gpu.renderer("big")
    for i, kw in enumerate(({}, {kind: True}, {})):
        got, c = gpu.trace(monkeypatch, r, None, **kw)
        gpu.check(monkeypatch, "big", got, f"{kind} step {i}")
        if c is not None:
            assert int(c.walk) == gpu.abi.WALK_HYBRID and int(c.walk_instrumented) != gpu.abi.WALK_HYBRID


# ---- partial calls

def tile_rows(mask_rows, h):
    rows = np.zeros(h, bool)
    for t in mask_rows:
        rows[8 * t:8 * t + 8] = True
    return rows


@pytest.mark.timeout(120)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["big", "odd"])
def test_partial_calls_then_the_full_map(gpu, monkeypatch, name, order):
    """Rows [0, h), band (1, 3), a call without a tile row (nothing is launched), a trace over cleared intervals (no live
    ray) and a consuming trace, each followed by the full map.  A partial call writes its rows and no other."""
    t, oracle = gpu.torch, gpu.oracle
    r, b = gpu.renderer(name), TS.built(gpu.oracle, name)
    tiles = -(-b.sd_h // 8)
    h = b.sd_h // 16 * 8
    assert 0 < h < b.sd_h and h % 8 == 0 and tiles > 3
    sentinel = TS.bits(sentinel_array(b.want.shape, np.float32))

    def partial(rows, what, call):
        gpu.env(monkeypatch, {})
        gpu.prepare(r)
        call()
        t.cuda.synchronize()
        got = TS.bits(r.sd.cpu().numpy())
        assert np.array_equal(got[:, rows], TS.bits(b.want)[:, rows]), what
        assert np.array_equal(got[:, ~rows], sentinel[:, ~rows]), f"{what}: rows outside the call were written"

    def cleared():
        gpu.env(monkeypatch, {})
        gpu.prepare(r)
        r.clear_intervals()
        r.sd_trace()
        t.cuda.synchronize()
        assert np.array_equal(TS.bits(r.sd.cpu().numpy()), TS.bits(b.want_cleared(oracle))), "cleared intervals"

    def consume():
        got, _ = gpu.trace(monkeypatch, r, None, consume=True)
        gpu.check(monkeypatch, name, got, "consuming trace")
        iv = r.ray_minmax.cpu().numpy().view(np.uint32)
        assert (iv[0] == TS.CLEARED_MIN).all() and (iv[1] == TS.CLEARED_MAX).all(), "the intervals were not consumed"

    steps = [
        ("rows", lambda: partial(np.arange(b.sd_h) < h, f"rows [0, {h})", lambda: r.sd_trace_rows((0, h)))),
        ("band", lambda: partial(tile_rows(range(1, tiles, 3), b.sd_h), "band (1, 3)", lambda: r.sd_trace(band=(1, 3)))),
        ("no tile row", lambda: partial(np.zeros(b.sd_h, bool), "a band without a tile row",
                                        lambda: r.sd_trace(band=(tiles, tiles + 1)))),
        ("cleared", cleared),
        ("consume", consume),
    ]
    for what, step in ordered(steps, order):
        step()
        got, _ = gpu.trace(monkeypatch, r)
        gpu.check(monkeypatch, name, got, f"the full map after '{what}' ({order})")


# ---- clean tiles across sizes

@pytest.mark.timeout(120)
@pytest.mark.parametrize("order", ORDERS)
def test_clean_tiles_of_two_sizes_share_a_workspace(gpu, monkeypatch, order):
    """Two renderers with clean tiles, BIG and SMALL, alternating over one scene: the stamps are per renderer, the
    workspace is shared.  On a renderer's later visits the texels the oracle has a hit in are filled with the sentinel
    (their rays are live: they must be rewritten); the others hold the DEFAULT_DEPTH the first visit left, which a trace
    need not store again where no ray is live (an unbounded ray behind the far plane is not)."""
    t = gpu.torch
    rs = {}
    for name in TS.SEQUENCES["clean_tiles"]:
        rs[name] = gpu.new_renderer(name)
        rs[name].keep_clean_tiles()
    gpu.env(monkeypatch, {})
    for visit in range(3):
        for name in ordered(TS.SEQUENCES["clean_tiles"], order):
            r, b = rs[name], TS.built(gpu.oracle, name)
            r.ray_minmax.copy_(r.saved)
            if visit == 0:
                r.sd.view(t.uint8).fill_(SENTINEL)
            else:
                hit = (TS.bits(b.want) != TS.bits(b.default)).any(axis=(0, 3))
                r.sd.view(t.uint8)[:, t.from_numpy(hit).to(r.sd.device)] = SENTINEL
            c = r.sd_trace(counters=True) if visit == 2 else r.sd_trace()
            t.cuda.synchronize()
            assert np.array_equal(TS.bits(r.sd.cpu().numpy()), TS.bits(b.want)), (name, visit, order)
            if c is not None:
                assert int(c.texels_clean) > 0, "no tile was kept: the sequence did not reach the clean-tile path"


# ---- two streams over one scene

@pytest.mark.timeout(120)
@pytest.mark.parametrize("order", ORDERS)
def test_two_streams_over_one_scene(gpu, monkeypatch, order):
    """BIG on stream s1, SMALL on s2: alternating with a synchronize between the calls, then four calls each enqueued
    back to back and one synchronize.  Each stream has a workspace of its own; every map is the oracle's."""
    t = gpu.torch
    gpu.env(monkeypatch, {})
    names = ordered(TS.SEQUENCES["streams"], order)
    streams = {n: t.cuda.Stream() for n in names}
    assert len({s.cuda_stream for s in streams.values()} | {t.cuda.current_stream().cuda_stream}) == 3
    rs = {n: gpu.new_renderer(n) for n in names}
    for rep in range(2):
        for n in names:
            with t.cuda.stream(streams[n]):
                gpu.prepare(rs[n])
                rs[n].sd_trace()
            t.cuda.synchronize()
            gpu.check(monkeypatch, n, rs[n].sd.cpu().numpy(), f"stream of {n}, synchronised call {rep}")
    maps = []
    for rep in range(4):
        for n in names:
            with t.cuda.stream(streams[n]):
                rs[n].sd = t.empty_like(rs[n].sd)  # a map per call: all eight are read after the one synchronize
                rs[n].sd.view(t.uint8).fill_(SENTINEL)
                rs[n].sd_trace()
                maps.append((n, rep, rs[n].sd))
    t.cuda.synchronize()
    for n, rep, sd in maps:
        gpu.check(monkeypatch, n, sd.cpu().numpy(), f"stream of {n}, back-to-back call {rep}")


# ---- the workspace list wraps at 64 streams

def hip_runtime():
    """The HIP runtime this process has loaded (torch's)."""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime is loaded")


@pytest.mark.timeout(120)
def test_workspace_list_wraps(gpu, monkeypatch):
    """One scene traced once on each of 66 distinct streams, then again on the first: the 65th drains the device,
    releases every workspace and starts over.  torch's pooled streams first, the rest created on the HIP runtime."""
    from rsd.frame import GpuScene
    t = gpu.torch
    gpu.env(monkeypatch, {})
    count = 66
    pooled = [t.cuda.Stream(priority=p) for p in (0, -1) for _ in range(32)]
    handles = []
    for h in [t.cuda.current_stream().cuda_stream] + [s.cuda_stream for s in pooled]:
        if h not in handles:
            handles.append(h)
    handles = handles[:count]
    hip, created = hip_runtime(), []
    hip.hipStreamCreate.argtypes, hip.hipStreamDestroy.argtypes = [C.POINTER(C.c_void_p)], [C.c_void_p]
    gs = GpuScene(gpu.dev, TS.host_scene("arcade_tiny"))
    try:
        while len(handles) < count:
            s = C.c_void_p()
            assert hip.hipStreamCreate(C.byref(s)) == 0 and s.value
            created.append(s.value)
            if s.value not in handles:
                handles.append(s.value)
        assert len(set(handles)) == count, "the streams are not distinct"
        print(f"{count} streams: {count - len(created)} of torch's, {len(created)} created")
        r = gpu.new_renderer("small", gs)
        for i, h in enumerate(handles + handles[:1]):
            with t.cuda.stream(t.cuda.ExternalStream(h) if h else t.cuda.default_stream()):
                assert r.stream == h
                gpu.prepare(r)
                r.sd_trace()
            t.cuda.synchronize()
            assert np.array_equal(TS.bits(r.sd.cpu().numpy()), TS.bits(r.built.want)), f"trace {i} of {count + 1}"
    finally:
        t.cuda.synchronize()
        gs.release()
        for s in created:
            hip.hipStreamDestroy(s)


# ---- results-neutral knobs

# The persistent walks' blocks claim their rays with an atomic add on their partition's head and leave when the index
# passes the count the setup launch left (sd_trace_queue_body, sd_trace_row_body, the resolve kernel): no block waits for
# another, so a grid below the default (8 blocks per CU, 16 for the quad walk, 4 row blocks in the hybrid) is only slower.
# The blocks are single waves with 8 or 16 KB of LDS whatever their number: a larger grid queues, it is not refused.
NEUTRAL = {
    "pool256": dict(RSD_TRACE_POOL="256"),
    "prio": dict(RSD_TRACE_PRIO="on"),
    "rowprio": dict(RSD_TRACE_ROWPRIO="on"),
    "spread": dict(RSD_TRACE_SPREAD="on"),
    "lpt_absolute": dict(RSD_TRACE_LPT="0.5"),
    "lpt_relative": dict(RSD_TRACE_LPT="-0.25"),
    "waves_per_cu_below": dict(RSD_TRACE_WAVES_PER_CU="2"),
    "waves_per_cu_above": dict(RSD_TRACE_WAVES_PER_CU="12"),
    "hybrid_rowwpc_below": dict(RSD_TRACE_HYBRID_ROWWPC="1"),
    "hybrid_rowwpc_above": dict(RSD_TRACE_HYBRID_ROWWPC="6"),
    # the knobs above on the walks the default (the hybrid) does not take
    "spread_quad": dict(RSD_TRACE_SPREAD="on", RSD_TRACE_WALK="quad", RSD_TRACE_HYBRID="off"),
    "spread_fused": dict(RSD_TRACE_SPREAD="on", RSD_TRACE_WALK="fused", RSD_TRACE_HYBRID="off"),
    "waves_per_cu_quad": dict(RSD_TRACE_WAVES_PER_CU="3", RSD_TRACE_WALK="quad", RSD_TRACE_HYBRID="off"),
    "pool256_fused": dict(RSD_TRACE_POOL="256", RSD_TRACE_WALK="fused", RSD_TRACE_HYBRID="off"),
}


@pytest.mark.timeout(120)
@pytest.mark.parametrize("knob", list(NEUTRAL))
@pytest.mark.parametrize("name", ["big", "slivers"])
def test_neutral_knobs_keep_the_bits_and_the_walk(gpu, monkeypatch, name, knob):
    """The A/B options DESIGN calls results-neutral, each handed through sd_plan and sd_args to the kernels: the
    oracle's bits, and the walk of the call without the knob."""
    env = NEUTRAL[knob]
    base = {k: v for k, v in env.items() if k in ("RSD_TRACE_WALK", "RSD_TRACE_HYBRID")}
    r = gpu.renderer(name)
    _, plain = gpu.trace(monkeypatch, r, base, counters=True)
    got, _ = gpu.trace(monkeypatch, r, env)
    gpu.check(monkeypatch, name, got, f"{knob} on {name}", env)
    got, c = gpu.trace(monkeypatch, r, env, counters=True)
    assert int(c.walk) == int(plain.walk), (knob, gpu.abi.WALK_NAMES[int(c.walk)], gpu.abi.WALK_NAMES[int(plain.walk)])
    gpu.check(monkeypatch, name, got, f"{knob} on {name}, instrumented", env)
    if not base:
        assert int(plain.walk) == gpu.abi.WALK_HYBRID


# ---- device memory

MIB = 1 << 20
LEAK_CYCLES = 16


def free_bytes(torch):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


@pytest.mark.timeout(300)
def test_scene_release_returns_the_raster_scratch(gpu, monkeypatch):
    """16 cycles of upload -> raster-walk trace -> release of a scene whose raster scratch is measured first (an SD map of
    1024 x 1024 at K = 8), then one cycle of a dynamic, rigged scene that also runs RTAO and rebuilds its entry grid (every
    other allocation a scene owns): free device memory ends within 4 x the scratch of where it began -- a quarter of what
    16 leaked copies take; the margin is for the allocator's granularity and the process-wide tables that are never freed
    by design (the coverage tables)."""
    from rsd.animation import Rig
    from rsd.frame import FrameConfig, GpuScene, Renderer
    t, abi = gpu.torch, gpu.abi
    scene = TS.host_scene("arcade_tiny")
    cfg = FrameConfig(visible_w=896, visible_h=896, guard_band=0, divisor=1, sd_samples=4, max_count=8, sd_guard_px=64,
                      radius=1.0, numerics="exact")
    gs = GpuScene(gpu.dev, scene)
    r = Renderer(scene, cfg, dev=gpu.dev, gpu_scene=gs)
    assert (r.sd_w, r.sd_h) == (1024, 1024)
    gpu.env(monkeypatch, {})
    r.gbuffer()
    r.clear_intervals()
    r.pass1()
    t.cuda.synchronize()
    saved = r.ray_minmax.clone()
    r.sd_trace()   # the stream's workspace but for the raster scratch
    monkeypatch.setenv("RSD_TRACE_WALK", "raster")
    warm = free_bytes(t)
    r.sd_trace()
    scratch = warm - free_bytes(t)
    assert int(r.sd_trace(counters=True).walk) == abi.WALK_RASTER
    gs.release()
    assert scratch >= 32 * MIB, f"the raster scratch measures {scratch / MIB:.1f} MiB"

    before = free_bytes(t)
    for _ in range(LEAK_CYCLES):
        r.gscene = GpuScene(gpu.dev, scene)
        r.ray_minmax.copy_(saved)
        r.sd_trace()
        t.cuda.synchronize()
        r.gscene.release()
    # d_dyn, d_rig, d_rtao_table and a replaced d_entry
    ids = np.arange(0, scene.positions.shape[0], 7, dtype=np.uint32)
    m = np.zeros((ids.size, 4), np.uint32)
    w = np.tile(np.array([1, 0, 0, 0], np.float32), (ids.size, 1))
    r.gscene = GpuScene(gpu.dev, scene, dynamic=True)
    r.gscene.attach_rig(Rig(ids, m, w, 1))
    r.gscene.update_pose(np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], np.float32))
    r.gscene.rebuild_entry_grid()
    out = r.rtao(spp=1)
    r.ray_minmax.copy_(saved)
    r.sd_trace()
    t.cuda.synchronize()
    del out
    r.gscene.release()
    after = free_bytes(t)
    line = (f"raster scratch {scratch / MIB:.1f} MiB; free device memory {before / MIB:.1f} MiB before and "
            f"{after / MIB:.1f} MiB after {LEAK_CYCLES} + 1 cycles: a drop of {(before - after) / MIB:.1f} MiB "
            f"({(before - after) / scratch:.2f} x the scratch; {LEAK_CYCLES} leaked copies: {LEAK_CYCLES * scratch / MIB:.1f} MiB)")
    print(line)
    report("trace_state_device_memory", scratch_bytes=int(scratch), free_before=int(before), free_after=int(after),
           cycles=LEAK_CYCLES)
    assert before - after <= 4 * scratch, line
