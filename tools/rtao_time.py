"""GPU time of the RTAO kernel next to the G-buffer kernel at the same extent (diagnostics): HIP events around
rsd_gbuffer_raster -- one coherent primary ray per pixel, the yardstick -- and around rsd_rtao for each spp,
alternating in one process, the median and spread over --launches launches of each after a warm-up, for BASELINE
configs.  The world G-buffer that RTAO reads comes from rsd_gbuffer_world once per config; the frame index
advances with every launch, as in the graph pass.
usage: python tools/rtao_time.py [config ...] [--launches N] [--spp 1,4] [--max-t-hit T] [--out file.json]"""
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

OPTS = ("--launches", "--out", "--spp", "--max-t-hit")


def _opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def _stats(us):
    q = np.percentile(us, [25, 50, 75])
    return {"median_us": round(float(q[1]), 1), "iqr_us": [round(float(q[0]), 1), round(float(q[2]), 1)],
            "min_max_us": [round(float(us.min()), 1), round(float(us.max()), 1)]}


def main():
    skip = {i + 1 for i, a in enumerate(sys.argv) if a in OPTS}
    names = [a for i, a in enumerate(sys.argv) if i and i not in skip and not a.startswith("--")]
    names = names or ["bistro_1080p_full", "bistro_4k_full_n16"]  # 1080p and 4K frames of the same scene
    launches = int(_opt("--launches", 30))
    spps = [int(x) for x in _opt("--spp", "1,4").split(",")]
    max_t = float(_opt("--max-t-hit", 1.0))
    assert torch.cuda.is_available(), "rtao_time measures on the GPU"
    L, dev, scenes, results = abi.lib(), Device(0), {}, []
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for name in names:
        kw, sc = CONFIGS[name]
        cfg = FrameConfig(**kw)
        if sc not in scenes:
            s = make_scene(sc)
            scenes[sc] = (s, GpuScene(dev, s))
        scene, gs = scenes[sc]
        cam, W, H = make_camera(scene, cfg), cfg.fb_w, cfg.fb_h
        f32 = dict(dtype=torch.float32, device="cuda")
        d, nw, pw = torch.empty((H, W), **f32), torch.empty((H, W, 4), **f32), torch.empty((H, W, 4), **f32)
        amb, dist = torch.empty((H, W), **f32), torch.empty((H, W), **f32)
        frame = [0]

        def gbuffer():
            abi.check(L.rsd_gbuffer_raster(gs.h, C.byref(cam), W, H, cfg.cull_mode, p(d), p(nw), None), "gbuffer")

        def rtao(prm):
            abi.check(L.rsd_rtao(gs.h, C.byref(prm), W, H, p(pw), p(nw), frame[0], p(amb), p(dist), None, None), "rtao")
            frame[0] += 1

        abi.check(L.rsd_gbuffer_world(gs.h, C.byref(cam), W, H, cfg.cull_mode, p(d), p(nw), p(pw), None), "gbuffer_world")
        row = {"config": name, "scene": sc, "triangles": scene.triangle_count, "width": W, "height": H,
               "launches": launches, "max_t_hit": max_t,
               "background_fraction": round(float((torch.count_nonzero(pw[..., 3] == 0) / (W * H)).item()), 4)}
        for spp in spps:
            prm = abi.RTAOParams(spp=spp, max_t_hit=max_t)
            for _ in range(5):
                gbuffer()
                rtao(prm)
            torch.cuda.synchronize()
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(launches)]
            for e in ev:
                e[0].record()
                gbuffer()
                e[1].record()
                rtao(prm)
                e[2].record()
            torch.cuda.synchronize()
            t = np.array([[e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])] for e in ev]) * 1e3
            g, r = _stats(t[:, 0]), _stats(t[:, 1])
            occluded = float((torch.count_nonzero(amb < 1.0) / (W * H)).item())
            row[f"spp_{spp}"] = {"gbuffer_raster": g, "rtao": r,
                                 "rtao_over_gbuffer": round(r["median_us"] / g["median_us"], 3),
                                 "occluded_fraction": round(occluded, 4)}
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
