"""The CPU checker of the motion-vector tests (tests/native/mvec_ref.c): a brute-force statement of
rsd_gbuffer_motion's mvec / mvecW over the oracle's triangle test and alpha test, plus a float64 evaluation of the
same formula from the checker's winning hits.  Shared by tests/test_mvec.py (which pins it to the oracle),
tests/test_gpu_mvec.py and tests/test_gpu_graph_mvec.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
SIZES = [(75, 45), (13, 7)]  # partial 8x8 tiles on both axes; smaller than one 64 x 4 image block
SCENES = {"opaque": ("arcade_tiny", 3000), "alpha": ("foliage_small", 3000)}
MISS = 0xFFFFFFFF

_lib = None


def build(oracle, out_dir):
    """Compile the checker against the oracle's shared library (once per process)."""
    global _lib
    if _lib is None:
        olib = Path(oracle.build())
        so = Path(out_dir) / "libmvec_ref.so"
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-I", str(olib.parents[1]),
                        "-o", str(so), str(HERE / "native" / "mvec_ref.c"), str(olib),
                        f"-Wl,-rpath,{olib.parent}", "-lm"], check=True)
        oracle.lib()  # the oracle is loaded first: the checker binds to the same library
        L = C.CDLL(str(so))
        vp, u32 = C.c_void_p, C.c_uint32
        L.mvec_ref.restype = None
        L.mvec_ref.argtypes = [vp, C.c_int, vp, vp, vp, vp, u32, vp, vp, u32, u32, u32, vp, vp, vp, vp, C.c_int]
        _lib = L
    return _lib


def make_scene(kind):
    from rsd.scenes import make_scene as mk
    name, tris = SCENES[kind]
    return mk(name, target_tris=tris)


def camera(scene, size, pos=None, target=None):
    """librsd's camera of a guard-less frame of `size` on `scene`, optionally from another position / target."""
    from rsd.frame import FrameConfig, look_at
    cfg = FrameConfig(visible_w=size[0], visible_h=size[1], guard_band=0)
    c = scene.camera
    return look_at(pos if pos is not None else c["pos"], target if target is not None else c["target"], c["up"], cfg)


def moved(scene, seed, part=(0.4, 0.3, -0.5), jitter=0.02):
    """Per-vertex jitter of a fixed seed plus the last eighth of the triangles translated by `part`."""
    rng = np.random.default_rng(seed)
    p = scene.positions + (jitter * rng.standard_normal(scene.positions.shape)).astype(np.float32)
    v = np.unique(scene.indices[-max(1, scene.indices.shape[0] // 8):])
    p[v] += np.float32(part)
    return np.ascontiguousarray(p, np.float32)


def run(oracle, lib, scene, positions, prev_positions, cam, prev_cam, size, cull):
    """The checker on `scene`'s topology with the given current and previous positions; cam / prev_cam are librsd
    or oracle cameras.  Returns dict(mvec [H,W,2], mvec_w [H,W,4], prim [H,W] uint32 (MISS: no hit),
    tuv [H,W,3] = (t, bu, bv))."""
    from helpers import to_oracle
    W, H = size
    oc = cam if isinstance(cam, oracle.Camera) else to_oracle(cam, oracle.Camera)
    op = prev_cam if isinstance(prev_cam, oracle.Camera) else to_oracle(prev_cam, oracle.Camera)
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    prev = np.ascontiguousarray(prev_positions, np.float32).reshape(-1, 3)
    assert pos.shape == prev.shape == scene.positions.shape
    osc = oracle.Scene(pos, scene.indices, scene.flags, scene.alpha)
    out = dict(mvec=np.zeros((H, W, 2), np.float32), mvec_w=np.zeros((H, W, 4), np.float32),
               prim=np.zeros((H, W), np.uint32), tuv=np.zeros((H, W, 3), np.float32))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.mvec_ref(osc.h, int(scene.alpha is not None), p(pos), p(prev), p(osc.indices), p(osc.flags), len(osc.indices),
                 C.byref(oc), C.byref(op), W, H, cull, p(out["mvec"]), p(out["mvec_w"]), p(out["prim"]),
                 p(out["tuv"]), oracle.effective_cpus())
    return out


def _cam64(cam):
    g = lambda n: np.array(list(getattr(cam, n)), np.float64)
    return dict(pos=g("posW"), U=g("U"), V=g("V"), W=g("W"), jx=float(cam.jitterX), jy=float(cam.jitterY))


def mvec_f64(hits, indices, positions, prev_positions, cam, prev_cam, size, prev_cam_offset=None):
    """The definition in float64 (numpy), from the checker's winning hits (`hits`: run()'s result, of which prim and
    tuv are read): positions / prev_positions may be float64.  prev_cam_offset: a float64 vector added to the previous
    camera's position.  Returns (mvec [H,W,2], mvec_w [H,W,3]); a miss is 0."""
    W, H = size
    c, pc = _cam64(cam), _cam64(prev_cam)
    if prev_cam_offset is not None:
        pc["pos"] = pc["pos"] + np.asarray(prev_cam_offset, np.float64)
    pos, prev = np.asarray(positions, np.float64), np.asarray(prev_positions, np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    u, v = (xs + 0.5) / W, (ys + 0.5) / H
    ndcx, ndcy = 2.0 * (u - c["jx"]) - 1.0, -2.0 * (v + c["jy"]) + 1.0
    d = ndcx[..., None] * c["U"] + ndcy[..., None] * c["V"] + c["W"]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    hit = hits["prim"] != MISS
    prim = np.where(hit, hits["prim"], 0).astype(np.int64)
    t, bu, bv = (hits["tuv"][..., k].astype(np.float64) for k in range(3))
    tri = np.asarray(indices, np.int64)[prim]  # [H, W, 3]
    dj = prev[tri] - pos[tri]                  # [H, W, 3 vertices, 3]
    b0 = (1.0 - bu) - bv
    D = b0[..., None] * dj[..., 0, :] + bu[..., None] * dj[..., 1, :] + bv[..., None] * dj[..., 2, :]
    P = c["pos"] + d * t[..., None]
    rel = (P + D) - pc["pos"]
    pa = rel @ (pc["U"] / (pc["U"] @ pc["U"]))
    pb = rel @ (pc["V"] / (pc["V"] @ pc["V"]))
    pw = rel @ (pc["W"] / (pc["W"] @ pc["W"]))
    front = pw > 0.0
    safe = np.where(front, pw, 1.0)
    mv = np.stack([np.where(front, (pa / safe + 1.0) * 0.5 - u, 2.0), np.where(front, (1.0 - pb / safe) * 0.5 - v, 2.0)],
                  -1)
    return np.where(hit[..., None], mv, 0.0), np.where(hit[..., None], D, 0.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
