"""GPU time of the raster stochastic depth map (rsd_sd_raster) next to the ray-traced one (rsd_sd_trace) on
the same frame (diagnostics): HIP events around each, alternating in one process, the median over --launches
launches of each after a warm-up, for BASELINE configs.  Each producer reads the intervals of its own pass 1
on the same G-buffer: the RT map with the config's SD guard band and jitter, the raster map without either
(SVAO.cpp:229, :721), with linearize, Alpha = 1.5 / N and the stencil from rayMax, as SVAO's raster mode runs it.
usage: python tools/sd_raster_time.py [config ...] [--launches N] [--out file.json]"""
import ctypes as C
import dataclasses
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "ray-traced-stochastic-depth-map_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rsd import abi  # noqa: E402
from rsd.frame import CONFIGS, Device, FrameConfig, GpuScene, Renderer  # noqa: E402
from rsd.scenes import make_scene  # noqa: E402


def _opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    skip = {i + 1 for i, a in enumerate(sys.argv) if a in ("--launches", "--out")}
    names = [a for i, a in enumerate(sys.argv) if i and i not in skip and not a.startswith("--")]
    names = names or ["suntemple_1080p_q"]  # BASELINE configs[1]
    launches = int(_opt("--launches", 30))
    assert torch.cuda.is_available(), "sd_raster_time measures on the GPU"
    dev, scenes, results = Device(0), {}, []
    for name in names:
        kw, sc = CONFIGS[name]
        cfg = FrameConfig(**kw)
        if sc not in scenes:
            s = make_scene(sc)
            scenes[sc] = (s, GpuScene(dev, s))
        scene, gs = scenes[sc]
        rt = Renderer(scene, cfg, gpu_scene=gs, dev=dev)
        ra = Renderer(scene, dataclasses.replace(cfg, sd_guard_px=0, jitter=False), gpu_scene=gs, dev=dev)
        for r in (rt, ra):
            r.gbuffer()
            r.clear_intervals()
            r.pass1()
        ra.sd_raster()  # renders ra.raster_depth; the timed calls below reuse it
        prm = abi.SDRasterParams(sample_count=cfg.sd_samples, alpha=float(np.float32(1.5 / cfg.sd_samples)),
                                 cull_mode=cfg.cull_mode, linearize=True, alpha_test=cfg.alpha_test,
                                 implementation=cfg.implementation, ray_interval=cfg.ray_interval, use_stencil=True)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

        def raster():
            abi.check(abi.lib().rsd_sd_raster(gs.h, C.byref(ra.cam), C.byref(prm), p(ra.raster_depth), cfg.fb_w,
                                              cfg.fb_h, p(ra.ray_min), p(ra.ray_max), None, p(ra.sd), ra.sd_w, ra.sd_h,
                                              None), "rsd_sd_raster")

        for _ in range(5):
            rt.sd_trace()
            raster()
        torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(launches)]
        for e in ev:
            e[0].record()
            rt.sd_trace()
            e[1].record()
            raster()
            e[2].record()
        torch.cuda.synchronize()
        t = np.array([[e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])] for e in ev]) * 1e3
        t_us, r_us = float(np.median(t[:, 0])), float(np.median(t[:, 1]))
        row = {"config": name, "scene": sc, "triangles": scene.triangle_count, "sd_samples": cfg.sd_samples,
               "launches": launches,
               "sd_trace": {"sd_size": [rt.sd_w, rt.sd_h], "us": round(t_us, 1),
                            "min_max_us": [round(float(t[:, 0].min()), 1), round(float(t[:, 0].max()), 1)],
                            "texels_without_ray": round(float((rt.ray_max == 0).float().mean().item()), 4)},
               "sd_raster": {"sd_size": [ra.sd_w, ra.sd_h], "us": round(r_us, 1),
                             "min_max_us": [round(float(t[:, 1].min()), 1), round(float(t[:, 1].max()), 1)],
                             "stencilled_out": round(float((ra.ray_max == 0).float().mean().item()), 4),
                             "samples_written": round(float((ra.sd < 1.0).float().mean().item()), 4)},
               "raster_over_trace": round(r_us / t_us, 3)}
        print(json.dumps(row), flush=True)
        results.append(row)
    out = _opt("--out", None)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(json.dumps(results, indent=1))
    for _, gs in scenes.values():
        gs.release()
    dev.close()


if __name__ == "__main__":
    main()
