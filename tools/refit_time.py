"""GPU time of a dynamic-scene update next to what it replaces and what it costs afterwards (diagnostics), for
BASELINE configs.  The scene is uploaded as a dynamic one and its vertices are displaced by a small per-vertex
offset of a fixed seed.  Recorded per config:
  update_us             rsd_scene_update_positions from a device pointer (copy + records + refit launches), HIP events,
                        warm, the median over --launches updates alternating between the two position sets
  update_subset_us      rsd_scene_update_subset of 1 % of the vertices (the refit still covers the whole tree)
  upload_ms             rsd_scene_upload of the moved scene on the same box (wall clock; build_ms: its host build alone)
  rebuild_entry_grid_ms rsd_scene_rebuild_entry_grid after the update (wall clock)
  sd_trace_us           the SD trace of one frame: on the fresh upload, after the refit with the stale entry grid
                        dropped, and after the grid's rebuild (HIP events, warm, median)
usage: python tools/refit_time.py [config ...] [--launches N] [--amplitude A] [--out file.json]"""
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


def _median_us(fn, launches, warm=5):
    for _ in range(warm):
        fn(0)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(i)
        b.record()
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) for a, b in ev]) * 1e3
    return {"median": round(float(np.median(t)), 1), "min": round(float(t.min()), 1), "max": round(float(t.max()), 1)}


def main():
    skip = {i + 1 for i, a in enumerate(sys.argv) if a in ("--launches", "--out", "--amplitude")}
    names = [a for i, a in enumerate(sys.argv) if i and i not in skip and not a.startswith("--")]
    names = names or ["bistro_1080p_full", "bistro_4k_full_n16"]  # BASELINE configs[1] and configs[4]
    launches, amplitude = int(_opt("--launches", 30)), float(_opt("--amplitude", 0.01))
    assert torch.cuda.is_available(), "refit_time measures on the GPU"
    dev, scenes, results = Device(0), {}, []
    for name in names:
        kw, sc = CONFIGS[name]
        cfg = FrameConfig(**kw)
        if sc not in scenes:
            s = make_scene(sc)
            rng = np.random.default_rng(17)
            p1 = np.ascontiguousarray(s.positions + (amplitude * rng.standard_normal(s.positions.shape)).astype(np.float32))
            t0 = time.perf_counter()
            fresh = GpuScene(dev, dataclasses.replace(s, positions=p1))
            upload_ms = (time.perf_counter() - t0) * 1e3
            scenes[sc] = dict(scene=s, p1=p1, fresh=fresh, upload_ms=upload_ms, dyn=GpuScene(dev, s, dynamic=True))
        e = scenes[sc]
        s, p1, fresh, dyn = e["scene"], e["p1"], e["fresh"], e["dyn"]
        moved = dataclasses.replace(s, positions=p1)
        d0, d1 = torch.from_numpy(s.positions).cuda(), torch.from_numpy(p1).cuda()
        nv = s.positions.shape[0]
        ids = torch.from_numpy(np.random.default_rng(18).choice(nv, max(1, nv // 100), replace=False).astype(np.int32)).cuda()
        sub = d1[ids.long()].contiguous()

        def trace_us(gs):
            r = Renderer(moved, cfg, dev=dev, gpu_scene=gs)
            r.gbuffer()
            r.clear_intervals()
            r.pass1()
            return _median_us(lambda i: r.sd_trace(), launches)

        row = {"config": name, "scene": sc, "triangles": s.triangle_count, "vertices": nv, "nodes": dyn.info.node_count,
               "amplitude": amplitude, "launches": launches, "upload_ms": round(e["upload_ms"], 1),
               "build_ms": round(fresh.info.build_ms, 1), "dynamic_bytes": int(dyn.dynamic_info().dynamic_bytes)}
        row["update_us"] = _median_us(lambda i: dyn.update_positions(d1 if i % 2 == 0 else d0), launches)
        row["update_subset_us"] = _median_us(lambda i: dyn.update_subset(ids, sub), launches)
        row["sd_trace_us"] = {"fresh_upload": trace_us(fresh)}
        dyn.update_positions(d1)
        assert dyn.dynamic_info().entry_grid_current == 0
        row["sd_trace_us"]["refit_grid_dropped"] = trace_us(dyn)
        t0 = time.perf_counter()
        dyn.rebuild_entry_grid()
        row["rebuild_entry_grid_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        row["sd_trace_us"]["refit_grid_rebuilt"] = trace_us(dyn)
        dyn.update_positions(d0)  # the next config starts from the upload's positions
        torch.cuda.synchronize()
        print(json.dumps(row), flush=True)
        results.append(row)
    out = _opt("--out", str(ROOT / "profiles" / "refit" / "refit_time.json"))
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(results, indent=1) + "\n")
    for e in scenes.values():
        e["fresh"].release()
        e["dyn"].release()
    dev.close()


if __name__ == "__main__":
    main()
