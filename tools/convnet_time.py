"""GPU time of rsd_convnet_run (diagnostics): HIP events around the fused kernel and the per-layer kernels
(RSD_CONVNET_FUSED=off, read by every run), each with fast and exact numerics, and around rsd_ao_guided_blur (R = 2, both
passes) on the same layers as the yardstick, alternating in one process; the median and spread over --launches launches
of each after a warm-up.  The net is a seeded 3 x 3 4 -> 8 -> 8 -> 1 net with distinct weights per slice; the inputs are
seeded random R8Unorm bright / dark / importance and R32Float depth layers of the config's frame size -- the kernels'
time does not depend on the values.  FLOPs count 2 per multiply-add of every layer on every texel inside the scissor,
of the last layer channel 0 only (what is computed); the peak is 157.3 TF FP32.
usage: python tools/convnet_time.py [config ...] [--launches N] [--guard-band G] [--out file.json]
       (--out defaults to profiles/convnet/convnet_time.json)"""
import ctypes as C
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "ray-traced-stochastic-depth-map_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rsd import abi  # noqa: E402
from rsd.convnet import ConvNet  # noqa: E402
from rsd.frame import CONFIGS, FrameConfig  # noqa: E402

OPTS = ("--launches", "--out", "--guard-band")
PEAK_FP32_TFLOPS = 157.3
CHANNELS = [4, 8, 8, 1]
KERNEL = 3


def _opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def _stats(us):
    q = np.percentile(us, [25, 50, 75])
    return {"median_us": round(float(q[1]), 1), "iqr_us": [round(float(q[0]), 1), round(float(q[2]), 1)],
            "min_max_us": [round(float(us.min()), 1), round(float(us.max()), 1)]}


def seeded_net(slices=16, seed=0):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 1 / np.sqrt(ci * KERNEL * KERNEL), (slices, KERNEL, KERNEL, ci, co)).astype(np.float32),
             rng.normal(0.05, 0.1, (slices, co)).astype(np.float32)) for ci, co in zip(CHANNELS[:-1], CHANNELS[1:])]


def main():
    skip = {i + 1 for i, a in enumerate(sys.argv) if a in OPTS}
    names = [a for i, a in enumerate(sys.argv) if i and i not in skip and not a.startswith("--")]
    names = names or ["bistro_1080p_full"]  # BASELINE configs[1]: a 2048 x 1208 frame, 16 layers of 512 x 302
    launches = int(_opt("--launches", 30))
    assert torch.cuda.is_available(), "convnet_time measures on the GPU"
    L, results = abi.lib(), []
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    net = ConvNet.from_arrays(seeded_net())
    for name in names:
        cfg = FrameConfig(**CONFIGS[name][0])
        guard, W, H = int(_opt("--guard-band", cfg.guard_band)), cfg.fb_w, cfg.fb_h
        qw, qh = (W + 3) // 4, (H + 3) // 4
        gen = torch.Generator(device="cuda").manual_seed(1)
        u8 = lambda: torch.randint(0, 256, (16, qh, qw), dtype=torch.uint8, device="cuda", generator=gen)  # noqa: E731
        bright, dark, importance = u8(), u8(), u8()
        depth = torch.rand((16, qh, qw), dtype=torch.float32, device="cuda", generator=gen)
        ao2 = torch.stack([bright, dark], -1).contiguous()
        out = torch.zeros((16, qh, qw), dtype=torch.float32, device="cuda")
        prm = {n: abi.ConvNetParams(W, H, 16, guard, numerics=v) for n, v in (("fast", 0), ("exact", 1))}
        scratch = torch.empty(net.scratch_bytes(prm["fast"]), dtype=torch.uint8, device="cuda")
        ping4, blurred = torch.empty((16, qh, qw, 4), dtype=torch.uint8, device="cuda"), torch.zeros((16, qh, qw), dtype=torch.uint8, device="cuda")
        g2 = abi.AOGuidedBlurParams(W, H, 16, 2, 2, True, guard)

        def convnet(numerics, fused):
            def call():
                if fused:
                    os.environ.pop("RSD_CONVNET_FUSED", None)
                else:
                    os.environ["RSD_CONVNET_FUSED"] = "off"
                abi.check(L.rsd_convnet_run(net.h, C.byref(prm[numerics]), p(bright), p(dark), p(importance), p(depth),
                                            p(scratch), p(out), None), "rsd_convnet_run")
            return call

        calls = {
            "fused_fast": convnet("fast", True), "per_layer_fast": convnet("fast", False),
            "fused_exact": convnet("exact", True), "per_layer_exact": convnet("exact", False),
            "guided_blur_r2": lambda: abi.check(L.rsd_ao_guided_blur(C.byref(g2), p(ao2), p(depth), p(ping4), p(blurred), None), "guided"),
        }
        for _ in range(5):
            for f in calls.values():
                f()
        torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)] for _ in range(launches)]
        for e in ev:
            e[0].record()
            for k, f in enumerate(calls.values()):
                f()
                e[k + 1].record()
        torch.cuda.synchronize()
        os.environ.pop("RSD_CONVNET_FUSED", None)
        t = np.array([[e[k].elapsed_time(e[k + 1]) for k in range(len(calls))] for e in ev]) * 1e3
        g = guard // 4
        texels = 16 * (qw - 2 * g) * (qh - 2 * g)
        couts = CHANNELS[1:-1] + [1]
        flop = 2 * texels * sum(KERNEL * KERNEL * ci * co for ci, co in zip(CHANNELS[:-1], couts))
        row = {"config": name, "width": W, "height": H, "layers": 16, "layer_width": qw, "layer_height": qh,
               "launches": launches, "guard_band": guard, "net": f"{KERNEL}x{KERNEL} " + "->".join(map(str, CHANNELS)),
               "fused_path_taken": bool(net.fused), "flop": flop, "peak_fp32_tflops": PEAK_FP32_TFLOPS}
        for k, label in enumerate(calls):
            row[label] = _stats(t[:, k])
            if label != "guided_blur_r2":
                tf = flop / (row[label]["median_us"] * 1e-6) / 1e12
                row[label]["tflops"] = round(tf, 2)
                row[label]["fraction_of_peak"] = round(tf / PEAK_FP32_TFLOPS, 4)
        print(json.dumps(row), flush=True)
        results.append(row)
    out_path = Path(_opt("--out", ROOT / "profiles" / "convnet" / "convnet_time.json"))
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(results, indent=1))
    net.close()


if __name__ == "__main__":
    main()
