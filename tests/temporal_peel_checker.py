"""The CPU checker of the TemporalDepthPeel tests (tests/native/temporal_peel_ref.c): a scalar restatement of
rsd_temporal_depth_peel that shares no code with the kernel, and the synthetic inputs both test files run.
Shared by tests/test_temporal_peel.py (known answers, input conditions) and tests/test_gpu_temporal_peel.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
F = np.float32

# the flag word of temporal_peel_ref.c
EXIT_MASK, EXIT_UV, EXIT_Z, EXIT_ITER = 3, 1, 2, 3
CLIPPED, POINT, QUIRK0, BEST_ZERO, CLIP_CAP, OFFSCREEN, ON_BOUND = 4, 8, 16, 32, 64, 128, 256

SIZES = [(150, 90), (75, 45)]  # more than one 64 x 4 block both ways; the second ragged on both axes
SEPARATIONS = [0.5, 0.05, 0.0]
ITERATIONS = [1, 7, 32]
POSES = ["step", "turn"]
SENTINEL = F(-7.0)

_lib = None


def build(out_dir):
    """Compile the checker (once per process): gcc, no contraction, SSE arithmetic."""
    global _lib
    if _lib is None:
        so = Path(out_dir) / "libtemporal_peel_ref.so"
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-msse2", "-mfpmath=sse", "-shared", "-fPIC", "-o", str(so),
                        str(HERE / "native" / "temporal_peel_ref.c"), "-lm"], check=True)
        L = C.CDLL(str(so))
        vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
        L.temporal_peel_ref.restype = None
        L.temporal_peel_ref.argtypes = [vp, vp, u32, u32, f32, f32, f32, f32, vp, vp, f32, C.c_int32, vp, vp, vp]
        _lib = L
    return _lib


def peel(lib, linear_z, prev_depth2, cam, c2p, p2c, min_separation, max_iterations, first_sample=None):
    """(depth2, flags) of the checker; cam: anything with farZ, frameWidth, frameHeight, focalLength.
    first_sample: an (H, W, 3) float32 array that receives (u, v, zRef) of each pixel's first search sample."""
    z = np.ascontiguousarray(linear_z, F)
    prev = np.ascontiguousarray(prev_depth2, F)
    assert z.ndim == 2 and prev.shape == z.shape
    c2p, p2c = np.ascontiguousarray(c2p, F).reshape(16), np.ascontiguousarray(p2c, F).reshape(16)
    out, flags = np.zeros_like(z), np.zeros(z.shape, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.temporal_peel_ref(p(z), p(prev), z.shape[1], z.shape[0], cam.farZ, cam.frameWidth, cam.frameHeight,
                          cam.focalLength, p(c2p), p(p2c), float(min_separation), int(max_iterations), p(out), p(flags),
                          p(first_sample) if first_sample is not None else None)
    return out, flags


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def shares(flags, out, z):
    """The share of pixels in each class the input conditions name."""
    n = flags.size
    ex = flags & EXIT_MASK
    return {"moved": float((bits(out) != bits(z)).sum() / n), "kept": float((bits(out) == bits(z)).sum() / n),
            "exit_uv": float((ex == EXIT_UV).sum() / n), "exit_z": float((ex == EXIT_Z).sum() / n),
            "exit_iter": float((ex == EXIT_ITER).sum() / n), "clipped": float(((flags & CLIPPED) != 0).sum() / n),
            "point": float(((flags & POINT) != 0).sum() / n), "quirk0_px": int(((flags & QUIRK0) != 0).sum()),
            "best_zero": float(((flags & BEST_ZERO) != 0).sum() / n), "clip_cap_px": int(((flags & CLIP_CAP) != 0).sum()),
            "offscreen": float(((flags & OFFSCREEN) != 0).sum() / n)}


def sequence_poses(scene, frames=4):
    """Look-at poses of the rendered sequence: the scene's camera moving sideways and up, a step large enough
    that surfaces seen in one frame are hidden in the next."""
    pos0, tgt0 = np.array(scene.camera["pos"], np.float64), np.array(scene.camera["target"], np.float64)
    step = np.array([0.35, 0.12, -0.1])
    return [((pos0 + step * i).tolist(), (tgt0 + 0.3 * step * i).tolist(), list(scene.camera["up"]))
            for i in range(frames)]


def boundary_case():
    """A layer at depth + min_separation to within rounding: identity matrices (the ray is a point, its one sample a
    zlerp of equal texels, the way back an identity), a flat first layer at 4 and a flat history at 4.5.  The
    sample comes back at 4.5 give or take an ulp or two, so the frame holds pixels exactly on the bound of the strict
    `>` test (flag ON_BOUND: not written), pixels just behind it (written) and pixels just in front (not written).
    Returns (cam, z, history, identity)."""
    from rsd.frame import FrameConfig, look_at
    cam = look_at([0.0, 2.0, 8.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0], FrameConfig(visible_w=150, visible_h=90, guard_band=0))
    z = np.full((90, 150), 4.0, F)
    return cam, z, (z + F(0.5)).astype(F), np.eye(4, dtype=F)


def synthetic(lib, width, height, pose):
    """One synthetic input: the current camera c1, the previous camera (pose "step": a small step away,
    as in test_temporal_ao_synthetic_parity; pose "turn": turned far enough for rays to leave its screen),
    random linearZ in [2, 12] and a previous second-layer map that holds, on random 6 x 6 blocks, a layer 0.2 - 3
    units behind linearZ (zero elsewhere: no information), with patches at 0, farZ, 0.995 farZ and equal to the
    first layer.  One flat patch of linearZ (depth 5) faces a smooth previous layer placed, with the checker's
    own first-sample positions at the default separation 0.5, where those pixels' rays meet it at their first
    sample: the only way to the search's `minSeparationDist * 0.001` exit, which noise never reaches.
    Returns dict(cam, prev_cam, z, prev2, c2p, p2c)."""
    from rsd.frame import FrameConfig, look_at
    from rsd.temporal import cur_view_to_prev_view, prev_view_to_cur_view
    rng = np.random.default_rng(width * 1000 + height + (7 if pose == "turn" else 0))
    cfg = FrameConfig(visible_w=width, visible_h=height, guard_band=0)
    cam = look_at([0.2, 2.1, 7.7], [0.1, 1.0, 0.0], [0.0, 1.0, 0.0], cfg)
    if pose == "step":
        prev_cam = look_at([0.0, 2.0, 8.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0], cfg)
    else:
        prev_cam = look_at([-0.4, 2.3, 8.2], [2.4, 0.2, 0.0], [0.0, 1.0, 0.0], cfg)
    H, W = height, width
    z = (2.0 + 10.0 * rng.random((H, W))).astype(F)
    ps = max(12, H // 4)  # the flat patch
    py, px = H // 3, W // 3
    z[py:py + ps, px:px + ps] = F(5.0)
    far = F(cam.farZ)
    behind = (z + rng.uniform(0.2, 3.0, (H, W))).astype(F)
    by, bx = (H + 5) // 6, (W + 5) // 6
    on = np.kron(rng.random((by, bx)) < 0.7, np.ones((6, 6), bool))[:H, :W]
    prev2 = np.where(on, behind, F(0.0)).astype(F)

    def patch(value, count, size):
        for _ in range(count):
            y, x = int(rng.integers(0, H - size)), int(rng.integers(0, W - size))
            prev2[y:y + size, x:x + size] = value if np.isscalar(value) else value[y:y + size, x:x + size]

    patch(F(0.0), 3, H // 6)
    patch(far, 4, H // 7)
    patch(F(0.995) * far, 4, H // 7)
    patch(z, 3, H // 6)
    # single far texels: footprints whose nearest texel is any of the four Gather components
    lone = rng.random((H, W)) < 0.02
    prev2[lone] = far
    c2p, p2c = cur_view_to_prev_view(cam, prev_cam), prev_view_to_cur_view(cam, prev_cam)
    # the layer the flat patch's rays meet at their first sample: a plane fitted to (u, v) -> zRef of those samples
    first = np.zeros((H, W, 3), F)
    peel(lib, z, prev2, cam, c2p, p2c, 0.5, 1, first_sample=first)
    s = first[py:py + ps, px:px + ps].reshape(-1, 3).astype(np.float64)
    coef = np.linalg.lstsq(np.c_[np.ones(len(s)), s[:, 0], s[:, 1]], s[:, 2], rcond=None)[0]
    x0, x1 = int(np.floor(s[:, 0].min() * W - 0.5)) - 1, int(np.floor(s[:, 0].max() * W - 0.5)) + 3
    y0, y1 = int(np.floor(s[:, 1].min() * H - 0.5)) - 1, int(np.floor(s[:, 1].max() * H - 0.5)) + 3
    x0, x1, y0, y1 = max(x0, 0), min(x1, W), max(y0, 0), min(y1, H)
    if x1 > x0 and y1 > y0:
        tu, tv = np.meshgrid((np.arange(x0, x1) + 0.5) / W, (np.arange(y0, y1) + 0.5) / H)
        prev2[y0:y1, x0:x1] = (coef[0] + coef[1] * tu + coef[2] * tv).astype(F)
    return dict(cam=cam, prev_cam=prev_cam, z=z, prev2=prev2, c2p=c2p, p2c=p2c)
