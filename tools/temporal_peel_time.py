"""GPU time of the TemporalDepthPeel kernel next to the DepthPeeling kernel on the same frames (diagnostics), and
how the two second layers compare.  A short camera orbit of a BASELINE config (default: configs[1], the
2048 x 1208 frame): every frame's linear depth comes from rsd_gbuffer_raster -> rsd_linearize_depth, the
temporal history is the previous frame's own output, so the search really runs.  Per frame, HIP events
around rsd_temporal_depth_peel and around rsd_depth_peel (linear output), alternating in one process, --launches
launches of each after a warm-up; the medians over all frames' launches are reported with their spread.
Nothing is gated.  The layers: the share of pixels where each producer finds a second layer (temporal:
depth2 != linearZ; traced: depth2 < farZ) and the share where both do and agree within 1 %.
usage: python tools/temporal_peel_time.py [config] [--frames N] [--launches N] [--path orbit120] [--out file.json]"""
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "ray-traced-stochastic-depth-map_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rsd import abi  # noqa: E402
from rsd.frame import CONFIGS, Device, FrameConfig, GpuScene, camera_path, look_at  # noqa: E402
from rsd.scenes import make_scene  # noqa: E402
from rsd.temporal import cur_view_to_prev_view, prev_view_to_cur_view  # noqa: E402

OPTS = ("--frames", "--launches", "--path", "--out")
SEP, ITERATIONS = 0.5, 32  # the pass's defaults


def _opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def _stats(us):
    q = np.percentile(us, [25, 50, 75])
    return {"median_us": round(float(q[1]), 1), "iqr_us": [round(float(q[0]), 1), round(float(q[2]), 1)],
            "min_max_us": [round(float(us.min()), 1), round(float(us.max()), 1)]}


def main():
    skip = {i + 1 for i, a in enumerate(sys.argv) if a in OPTS}
    names = [a for i, a in enumerate(sys.argv) if i and i not in skip and not a.startswith("--")]
    name = names[0] if names else "bistro_1080p_full"
    frames, launches = int(_opt("--frames", 6)), int(_opt("--launches", 20))
    assert torch.cuda.is_available(), "temporal_peel_time measures on the GPU"
    L, dev = abi.lib(), Device(0)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    kw, sc = CONFIGS[name]
    cfg = FrameConfig(**kw)
    scene = make_scene(sc)
    gs = GpuScene(dev, scene)
    W, H = cfg.fb_w, cfg.fb_h
    poses = camera_path(_opt("--path", "orbit120"))[:frames + 1]
    f32 = dict(dtype=torch.float32, device="cuda")
    d, nw, z = torch.empty((H, W), **f32), torch.empty((H, W, 4), **f32), torch.empty((H, W), **f32)
    hist, out, traced = torch.zeros((H, W), **f32), torch.empty((H, W), **f32), torch.empty((H, W), **f32)
    t_us, p_us, per_frame, prev_cam = [], [], [], None
    for i, pose in enumerate(poses):
        cam = look_at(*pose, cfg)
        abi.check(L.rsd_gbuffer_raster(gs.h, C.byref(cam), W, H, cfg.cull_mode, p(d), p(nw), None), "gbuffer")
        abi.check(L.rsd_linearize_depth(p(d), p(z), W * H, cam.nearZ, cam.farZ, None), "linearize")
        pc = prev_cam or cam
        c2p = np.ascontiguousarray(cur_view_to_prev_view(cam, pc), np.float32)
        p2c = np.ascontiguousarray(prev_view_to_cur_view(cam, pc), np.float32)

        def temporal():
            abi.check(L.rsd_temporal_depth_peel(p(z), p(hist), W, H, C.byref(cam), c2p.ctypes.data_as(C.c_void_p),
                                                p2c.ctypes.data_as(C.c_void_p), SEP, ITERATIONS, p(out), None),
                      "temporal_depth_peel")

        def peel():
            abi.check(L.rsd_depth_peel(gs.h, C.byref(cam), W, H, cfg.cull_mode, p(z), SEP, 1, p(traced), None), "peel")

        if i > 0:  # frame 0 only fills the history: its search reads zeros
            for _ in range(3):
                temporal()
                peel()
            torch.cuda.synchronize()
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(launches)]
            for e in ev:
                e[0].record()
                temporal()
                e[1].record()
                peel()
                e[2].record()
            torch.cuda.synchronize()
            t = np.array([[e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])] for e in ev]) * 1e3
            t_us.append(t[:, 0])
            p_us.append(t[:, 1])
            has_t, has_p = out != z, traced < cam.farZ
            agree = has_t & has_p & ((out - traced).abs() <= 0.01 * traced)
            n = float(W * H)
            per_frame.append({"frame": i, "temporal_us": round(float(np.median(t[:, 0])), 1),
                              "depth_peel_us": round(float(np.median(t[:, 1])), 1),
                              "temporal_layer": round(has_t.sum().item() / n, 4),
                              "traced_layer": round(has_p.sum().item() / n, 4),
                              "both": round((has_t & has_p).sum().item() / n, 4),
                              "both_within_1pct": round(agree.sum().item() / n, 4)})
        else:
            temporal()
        hist.copy_(out)
        torch.cuda.synchronize()
        prev_cam = cam
    t_all, p_all = np.concatenate(t_us), np.concatenate(p_us)
    row = {"config": name, "scene": sc, "triangles": scene.triangle_count, "width": W, "height": H,
           "frames": len(per_frame), "launches_per_frame": launches, "min_separation": SEP, "iterations": ITERATIONS,
           "temporal_depth_peel": _stats(t_all), "depth_peel": _stats(p_all),
           "temporal_over_traced": round(float(np.median(t_all) / np.median(p_all)), 3),
           # the least the kernel must move: linearZ and the history in once, depth2 out
           "algorithmic_bytes": 12 * W * H,
           "algorithmic_gb_per_s": round(12 * W * H / (float(np.median(t_all)) * 1e-6) / 1e9, 1),
           "per_frame": per_frame}
    print(json.dumps(row), flush=True)
    out_path = _opt("--out", None)
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(json.dumps(row, indent=1))
    gs.release()
    dev.close()


if __name__ == "__main__":
    main()
