"""GPU time of posing an animated scene (rsd_scene_update_pose) next to what the same motion cost before it existed,
on the stand-in scene of a BASELINE config (default bistro_1080p_full, configs[1]).  A rig of --matrices matrices with
four influences per vertex covers 1 %, 10 % and 100 % of the vertices (a random draw of a fixed seed).  HIP events,
warm, the median [min, max] of --launches calls alternating between two poses, one box.  Recorded per fraction:
  update_pose_host_us       rsd_scene_update_pose from a host matrix table (copy of matrix_count x 48 B + pose kernel +
                            record rewrite + refit)
  update_positions_host_us  rsd_scene_update_positions from a host pointer with the posed positions (tests/
                            skinning_checker.py): what the caller had to do for the same motion before
  update_pose_device_us     rsd_scene_update_pose from a device table (no copy)
  pose_kernel_us            the pose kernel alone, per matrix-table variant (RSD_POSE_TABLE=global: 16-byte loads
                            through L1; lds: the table staged in LDS per workgroup): update_pose from a device table on
                            a scene of the same vertices and ONE triangle, whose record rewrite and refit are two
                            one-workgroup launches, minus those two launches timed alone on it (launch_floor_us, an
                            empty rsd_scene_update_subset)
  pose_bytes                the kernel's stream traffic: 60 B per animated vertex (id 4, matrix ids 16, weights 16, rest
                            12, store 12) + the table once; hbm_floor_us = pose_bytes / --hbm-tbs (6.3 TB/s achievable)
usage: python tools/skinning_time.py [config] [--launches N] [--matrices M] [--hbm-tbs T] [--out file.json]"""
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "ray-traced-stochastic-depth-map_amd"), str(ROOT / "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import skinning_checker  # noqa: E402
from rsd.animation import Rig  # noqa: E402
from rsd.frame import CONFIGS, Device, GpuScene  # noqa: E402
from rsd.scenes import Scene, make_scene  # noqa: E402


def _opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def _median_us(fn, launches, warm=5):
    for i in range(warm):
        fn(i)
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
    flags = ("--launches", "--out", "--matrices", "--hbm-tbs")
    skip = {i + 1 for i, a in enumerate(sys.argv) if a in flags}
    names = [a for i, a in enumerate(sys.argv) if i and i not in skip and not a.startswith("--")]
    name = names[0] if names else "bistro_1080p_full"
    launches, nm, tbs = int(_opt("--launches", 30)), int(_opt("--matrices", 64)), float(_opt("--hbm-tbs", 6.3))
    assert torch.cuda.is_available(), "skinning_time measures on the GPU"
    dev = Device(0)
    scene = make_scene(CONFIGS[name][1])
    nv = scene.positions.shape[0]
    rng = np.random.default_rng(23)
    poses = [skinning_checker.random_matrices(rng, nm, translation=0.05) for _ in range(2)]
    for p in poses:  # near the identity: the scene stays where the refit's boxes were measured before
        p[:] = 0.98 * skinning_checker.identity_matrices(nm) + 0.02 * p
    d_poses = [torch.from_numpy(p).cuda() for p in poses]
    dyn = GpuScene(dev, scene, dynamic=True)
    # the same vertices under one triangle: update_pose on it is the pose kernel plus two one-workgroup launches
    bare = GpuScene(dev, Scene("bare", scene.positions, np.array([[0, 1, 2]], np.uint32), np.zeros(1, np.uint32),
                               scene.camera), dynamic=True)
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    none_p = torch.zeros((0, 3), dtype=torch.float32, device="cuda")
    rows = []
    for frac in (0.01, 0.1, 1.0):
        n = max(1, int(round(frac * nv)))
        ids = rng.choice(nv, n, replace=False).astype(np.uint32) if n < nv else rng.permutation(nv).astype(np.uint32)
        w = rng.uniform(0.05, 1.0, (n, 4)).astype(np.float32)
        w /= w.sum(axis=1, keepdims=True)
        rig = Rig(ids, rng.integers(0, nm, (n, 4)), w, nm)
        posed = [skinning_checker.posed(scene.positions, rig, p) for p in poses]
        dyn.attach_rig(rig)
        bare.attach_rig(rig)
        row = {"config": name, "scene": CONFIGS[name][1], "triangles": scene.triangle_count, "vertices": nv,
               "fraction": frac, "animated": n, "matrices": nm, "launches": launches,
               "rig_bytes": int(dyn.rig_info().rig_bytes)}
        row["update_pose_host_us"] = _median_us(lambda i: dyn.update_pose(poses[i % 2]), launches)
        row["update_positions_host_us"] = _median_us(lambda i: dyn.update_positions(posed[i % 2]), launches)
        row["update_pose_device_us"] = _median_us(lambda i: dyn.update_pose(d_poses[i % 2]), launches)
        row["launch_floor_us"] = _median_us(lambda i: bare.update_subset(none, none_p), launches)
        row["pose_kernel_us"] = {}
        prev = os.environ.get("RSD_POSE_TABLE")
        for variant in ("global", "lds"):
            os.environ["RSD_POSE_TABLE"] = variant
            t = _median_us(lambda i: bare.update_pose(d_poses[i % 2]), launches)
            row["pose_kernel_us"][variant] = {"with_floor": t,
                                              "kernel": round(t["median"] - row["launch_floor_us"]["median"], 1)}
        if prev is None:
            del os.environ["RSD_POSE_TABLE"]
        else:
            os.environ["RSD_POSE_TABLE"] = prev
        row["pose_bytes"] = 60 * n + 48 * nm
        row["hbm_floor_us"] = round(row["pose_bytes"] / (tbs * 1e12) * 1e6, 2)
        dyn.update_positions(scene.positions)
        torch.cuda.synchronize()
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = _opt("--out", str(ROOT / "profiles" / "skinning" / "skinning_time.json"))
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps({"command": "python tools/skinning_time.py " + " ".join(sys.argv[1:]),
                                     "hbm_tbs": tbs, "rows": rows}, indent=1) + "\n")
    dyn.release()
    bare.release()
    dev.close()


if __name__ == "__main__":
    main()
