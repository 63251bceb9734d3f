"""GPU time of rsd_scene_rebuild_bvh next to the upload it replaces, and what each tree costs to trace (diagnostics),
for a BASELINE config.  The scene is uploaded as a dynamic one and moved two ways, both of a fixed seed:
  small   every vertex jittered by --amplitude (0.01) x N(0, 1)
  large   the same jitter, and the vertices of the last quarter of the triangles translated by --shift (0.25) of the
          scene's extent along x, y and z
Recorded per motion:
  upload_ms       rsd_scene_upload of the moved scene on the same box (wall clock; build_ms: its host build alone)
  rebuild_ms      rsd_scene_rebuild_bvh of the moved dynamic scene, warm, median [min, max] over --launches calls:
                  device (HIP events around its launches, rsd_scene_rebuild_info.device_ms) and wall (the whole
                  synchronous call: allocation, read-back, frees)
  nodes, depth    of the SAH tree and of the rebuilt one
  sd_trace_us     the SD trace of one frame (HIP events, warm, median) on a fresh SAH upload, on the refitted tree
                  (stale grid dropped, then rebuilt) and on the rebuilt tree (grid dropped, then rebuilt)
usage: python tools/rebuild_time.py [config] [--launches N] [--amplitude A] [--shift S] [--out file.json]"""
import dataclasses
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "ray-traced-stochastic-depth-map_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rsd.frame import CONFIGS, Device, FrameConfig, GpuScene, Renderer  # noqa: E402
from rsd.scenes import make_scene  # noqa: E402


def _opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def _stat(t, digits=1):
    t = np.asarray(t, np.float64)
    return {"median": round(float(np.median(t)), digits), "min": round(float(t.min()), digits),
            "max": round(float(t.max()), digits)}


def _median_us(fn, launches, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return _stat(np.array([a.elapsed_time(b) for a, b in ev]) * 1e3)


def main():
    flags = ("--launches", "--out", "--amplitude", "--shift")
    skip = {i + 1 for i, a in enumerate(sys.argv) if a in flags}
    names = [a for i, a in enumerate(sys.argv) if i and i not in skip and not a.startswith("--")]
    name = (names or ["bistro_1080p_full"])[0]  # BASELINE configs[1]: the 2.8 M-triangle stand-in
    launches, amplitude, shift = int(_opt("--launches", 30)), float(_opt("--amplitude", 0.01)), float(_opt("--shift", 0.25))
    assert torch.cuda.is_available(), "rebuild_time measures on the GPU"
    dev = Device(0)
    kw, sc = CONFIGS[name]
    cfg = FrameConfig(**kw)
    s = make_scene(sc)
    rng = np.random.default_rng(17)
    jitter = (amplitude * rng.standard_normal(s.positions.shape)).astype(np.float32)
    extent = np.ptp(s.positions, axis=0).astype(np.float32)
    part = np.unique(s.indices[-(s.indices.shape[0] // 4):])
    motions = {"small": s.positions + jitter, "large": s.positions + jitter}
    motions["large"][part] += np.float32(shift) * extent
    results = []
    for motion, p in motions.items():
        p = np.ascontiguousarray(p, np.float32)
        moved = dataclasses.replace(s, positions=p)

        def trace_us(gs):
            r = Renderer(moved, cfg, dev=dev, gpu_scene=gs)
            r.gbuffer()
            r.clear_intervals()
            r.pass1()
            return _median_us(lambda: r.sd_trace(), launches)

        t0 = time.perf_counter()
        fresh = GpuScene(dev, moved)
        upload_ms = (time.perf_counter() - t0) * 1e3
        row = {"config": name, "scene": sc, "motion": motion, "amplitude": amplitude, "shift": shift if motion == "large" else 0.0,
               "triangles": s.triangle_count, "vertices": int(s.positions.shape[0]), "launches": launches,
               "upload_ms": round(upload_ms, 1), "build_ms": round(fresh.info.build_ms, 1),
               "sah": {"nodes": fresh.info.node_count, "wide_depth": fresh.info.wide_depth}}
        row["sd_trace_us"] = {"fresh_sah_upload": trace_us(fresh)}
        fresh.release()
        dyn = GpuScene(dev, s, dynamic=True)
        dyn.update_positions(torch.from_numpy(p).cuda())
        row["sd_trace_us"]["refit_grid_dropped"] = trace_us(dyn)
        t0 = time.perf_counter()
        dyn.rebuild_entry_grid()
        row["rebuild_entry_grid_ms"] = {"refit": round((time.perf_counter() - t0) * 1e3, 1)}
        row["sd_trace_us"]["refit_grid_rebuilt"] = trace_us(dyn)
        for _ in range(3):  # warm: code objects, the allocator
            dyn.rebuild_bvh()
        wall, device = [], []
        for _ in range(launches):
            t0 = time.perf_counter()
            dyn.rebuild_bvh()
            wall.append((time.perf_counter() - t0) * 1e3)
            device.append(dyn.rebuild_info().device_ms)
        row["rebuild_ms"] = {"device": _stat(device, 3), "wall": _stat(wall, 3)}
        row["lbvh"] = {"nodes": dyn.info.node_count, "wide_depth": dyn.info.wide_depth}
        assert dyn.dynamic_info().entry_grid_current == 0
        row["sd_trace_us"]["rebuilt_grid_dropped"] = trace_us(dyn)
        t0 = time.perf_counter()
        dyn.rebuild_entry_grid()
        row["rebuild_entry_grid_ms"]["rebuilt"] = round((time.perf_counter() - t0) * 1e3, 1)
        row["sd_trace_us"]["rebuilt_grid_rebuilt"] = trace_us(dyn)
        dyn.release()
        torch.cuda.synchronize()
        print(json.dumps(row), flush=True)
        results.append(row)
    out = _opt("--out", str(ROOT / "profiles" / "rebuild" / "rebuild_time.json"))
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(results, indent=1) + "\n")
    dev.close()


if __name__ == "__main__":
    main()
