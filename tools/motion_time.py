"""GPU time of the motion G-buffer next to the pair of launches it replaces (diagnostics), on the BASELINE configs[1]
stand-in scene at its frame size.  The scene is uploaded as a dynamic one that tracks its motion, and its vertices are
displaced by a small per-vertex offset of a fixed seed, so the motion path reads real differences.  Recorded:
  world_plus_mvec_raster_us  rsd_gbuffer_world + rsd_motion_vectors_raster, today's pair for depth, normal, posW, mvec
  gbuffer_world_us           rsd_gbuffer_world alone
  gbuffer_motion_us          rsd_gbuffer_motion, the single launch (depth, normal, posW, mvec, mvecW)
  begin_frame_us             rsd_scene_motion_begin_frame's copy kernel (an update precedes each, outside the timing)
HIP events, warm, median [min, max] of --launches, all in one run.
usage: python tools/motion_time.py [config] [--launches N] [--amplitude A] [--out file.json]"""
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "ray-traced-stochastic-depth-map_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rsd import abi  # noqa: E402
from rsd.frame import CONFIGS, Device, FrameConfig, GpuScene, make_camera  # noqa: E402
from rsd.scenes import make_scene  # noqa: E402


def _opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def _median_us(fn, launches, before=None, warm=5):
    """fn(i) between two events; before(i) runs ahead of the first event, outside the timing."""
    for i in range(warm):
        if before:
            before(i)
        fn(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for i, (a, b) in enumerate(ev):
        if before:
            before(i)
        a.record()
        fn(i)
        b.record()
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) for a, b in ev]) * 1e3
    return {"median": round(float(np.median(t)), 1), "min": round(float(t.min()), 1), "max": round(float(t.max()), 1)}


def main():
    skip = {i + 1 for i, a in enumerate(sys.argv) if a in ("--launches", "--out", "--amplitude")}
    names = [a for i, a in enumerate(sys.argv) if i and i not in skip and not a.startswith("--")]
    name = names[0] if names else "bistro_1080p_full"  # BASELINE configs[1]
    launches, amplitude = int(_opt("--launches", 30)), float(_opt("--amplitude", 0.01))
    assert torch.cuda.is_available(), "motion_time measures on the GPU"
    kw, sc = CONFIGS[name]
    cfg = FrameConfig(**kw)
    s = make_scene(sc)
    rng = np.random.default_rng(17)
    p1 = np.ascontiguousarray(s.positions + (amplitude * rng.standard_normal(s.positions.shape)).astype(np.float32))
    dev = Device(0)
    gs = GpuScene(dev, s, dynamic=True, motion=True)
    d0, d1 = torch.from_numpy(s.positions).cuda(), torch.from_numpy(p1).cuda()
    gs.update_positions(d1)  # previous positions: the upload's; current: p1
    W, H = cfg.fb_w, cfg.fb_h
    cam = make_camera(s, cfg)
    f32 = dict(dtype=torch.float32, device="cuda")
    depth, normal, pos = torch.empty((H, W), **f32), torch.empty((H, W, 4), **f32), torch.empty((H, W, 4), **f32)
    mvec, mvec_w = torch.empty((H, W, 2), **f32), torch.empty((H, W, 4), **f32)
    L, p = abi.lib(), lambda t: C.c_void_p(t.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def world(i):
        abi.check(L.rsd_gbuffer_world(gs.h, C.byref(cam), W, H, cfg.cull_mode, p(depth), p(normal), p(pos), stream()),
                  "rsd_gbuffer_world")

    def pair(i):
        world(i)
        abi.check(L.rsd_motion_vectors_raster(C.byref(cam), C.byref(cam), p(depth), W, H, p(mvec), stream()),
                  "rsd_motion_vectors_raster")

    def motion(i):
        abi.check(L.rsd_gbuffer_motion(gs.h, C.byref(cam), C.byref(cam), W, H, cfg.cull_mode, p(depth), p(normal), p(pos),
                                       p(mvec), p(mvec_w), stream()), "rsd_gbuffer_motion")

    row = {"config": name, "scene": sc, "triangles": s.triangle_count, "vertices": int(s.positions.shape[0]),
           "width": W, "height": H, "amplitude": amplitude, "launches": launches,
           "motion_bytes": int(gs.motion_info().motion_bytes)}
    row["world_plus_mvec_raster_us"] = _median_us(pair, launches)
    row["gbuffer_world_us"] = _median_us(world, launches)
    row["gbuffer_motion_us"] = _median_us(motion, launches)
    row["hit_pixels"] = int((depth < 1.0).sum())
    row["moving_pixels"] = int((mvec_w != 0).any(dim=-1).sum())
    snaps = gs.motion_info().snapshots
    row["begin_frame_us"] = _median_us(lambda i: gs.begin_frame(), launches,
                                       before=lambda i: gs.update_positions(d0 if i % 2 == 0 else d1))
    assert gs.motion_info().snapshots == snaps + launches + 5, "every timed begin_frame enqueued its copy"
    torch.cuda.synchronize()
    print(json.dumps(row), flush=True)
    out = _opt("--out", str(ROOT / "profiles" / "motion" / "motion_time.json"))
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps([row], indent=1) + "\n")
    gs.release()
    dev.close()


if __name__ == "__main__":
    main()
