"""The CPU checker of the HBAO tests (tests/native/hbao_ref.c): a scalar restatement of the reference's HBAO
pixel shader that shares no code with csrc/hbao.hip, its own MT19937 noise table, and the synthetic inputs both
test files run.  Shared by tests/test_hbao.py (known answers, input conditions) and tests/test_gpu_hbao.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
F = np.float32

# the flag word of hbao_ref.c
FAR, SMALL, SCISSORED, RAGGED, NAN_TAP, TIE = 1, 2, 4, 8, 16, 32
RECOMPUTE_SHIFT = 8

SINGLE, DUAL = 0, 1
SIZES = [(150, 90), (64, 48)]  # 38 x 23 layers, ragged both ways, two 64-wide runs per row; 16 x 12, exact
GUARDS = [0, 8]
EXPONENTS = [2.0, 1.7]
SENTINEL = 0x5A


def radii(height):
    """The three radii of the parity test for a frame of this height.  With the tests' camera (frame height 24,
    focal length 21, so imageScale.y = 4 / 7 and imageScale.x = imageScale.y * aspect) the radius in pixels of a
    texel at depth z is 0.875 * radius * height / z in both axes, and the synthetic depths lie in [2, 12]:
    radius 1 leaves every texel above one pixel, the middle radius puts the early out at z = 7 and the small
    one at z = 2.4."""
    return [1.0, 7.0 / (0.875 * height), 2.4 / (0.875 * height)]


_lib = None


def build(out_dir):
    """Compile the checker (once per process): gcc, no contraction, SSE arithmetic."""
    global _lib
    if _lib is None:
        so = Path(out_dir) / "libhbao_ref.so"
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-msse2", "-mfpmath=sse", "-shared", "-fPIC", "-o", str(so),
                        str(HERE / "native" / "hbao_ref.c"), "-lm"], check=True)
        L = C.CDLL(str(so))
        vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
        L.hbao_ref.restype = None
        L.hbao_ref.argtypes = [vp, vp, vp, u32, u32, f32, f32, f32, f32, vp, f32, f32, f32, u32, u32, vp, vp, vp]
        L.hbao_ref_noise.restype = None
        L.hbao_ref_noise.argtypes = [vp, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def noise_table(lib):
    """(table [16][4] float32, the first three raw MT19937(0) draws, theta of entry 0)."""
    table, first3, theta0 = np.zeros((16, 4), F), np.zeros(3, np.uint32), np.zeros(1, F)
    lib.hbao_ref_noise(_p(table), _p(first3), _p(theta0))
    return table, first3, float(theta0[0])


def deinterleave(img):
    """DeinterleaveTexture on the host: (H, W[, c]) -> (16, ceil(H/4), ceil(W/4)[, c]), zeros outside the source."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    qh, qw = (H + 3) // 4, (W + 3) // 4
    pad = np.zeros((4 * qh, 4 * qw) + img.shape[2:], img.dtype)
    pad[:H, :W] = img
    return np.ascontiguousarray(np.stack([pad[s // 4::4, s % 4::4] for s in range(16)]))


def interleave(layers, width, height):
    """InterleaveTexture on the host: (16, qh, qw[, c]) -> (height, width[, c])."""
    layers = np.asarray(layers)
    qh, qw = layers.shape[1:3]
    full = np.zeros((4 * qh, 4 * qw) + layers.shape[3:], layers.dtype)
    for s in range(16):
        full[s // 4::4, s % 4::4] = layers[s]
    return np.ascontiguousarray(full[:height, :width])


def hbao(lib, depth_layers, depth2_layers, normal_w, cam, radius=1.0, bias=0.1, exponent=2.0, depth_mode=SINGLE,
         guard_band=0, rand=None, fill=SENTINEL):
    """(ambient layers [16][qh][qw][2] uint8, flags [16][qh][qw] uint32) of the checker.  cam: anything with farZ,
    frameWidth, frameHeight, focalLength and viewMat; normal_w: (H, W, 4) float32, the frame size; texels
    outside the scissor keep `fill`."""
    n = np.ascontiguousarray(normal_w, F)
    H, W = n.shape[:2]
    qh, qw = (H + 3) // 4, (W + 3) // 4
    z = np.ascontiguousarray(depth_layers, F)
    assert z.shape == (16, qh, qw) and n.shape == (H, W, 4)
    z2 = None
    if depth_mode == DUAL:
        z2 = np.ascontiguousarray(depth2_layers, F)
        assert z2.shape == z.shape
    rand = noise_table(lib)[0] if rand is None else np.ascontiguousarray(rand, F)
    view = np.array(list(cam.viewMat), F)
    out, flags = np.full((16, qh, qw, 2), fill, np.uint8), np.zeros((16, qh, qw), np.uint32)
    lib.hbao_ref(_p(z), _p(z2) if z2 is not None else None, _p(n), W, H, cam.farZ, cam.frameWidth, cam.frameHeight,
                 cam.focalLength, _p(view), float(radius), float(bias), float(exponent), int(depth_mode),
                 int(guard_band), _p(rand), _p(out), _p(flags))
    return out, flags


def recompute_count(flags):
    return (flags >> RECOMPUTE_SHIFT) & 0xFF


def shares(flags):
    """The share of texels in each class the input conditions name (of all 16 layers' texels)."""
    n = flags.size
    far, small = (flags & FAR) != 0, (flags & SMALL) != 0
    shaded = ~far & ~small
    return {"far": float(far.sum() / n), "small": float(small.sum() / n), "shaded": float(shaded.sum() / n),
            "scissored_texels": int(((flags & SCISSORED) != 0).sum()), "ragged_texels": int(((flags & RAGGED) != 0).sum()),
            "nan_tap_texels": int(((flags & NAN_TAP) != 0).sum()),
            "recompute_of_shaded": float((recompute_count(flags)[shaded] > 0).sum() / max(1, shaded.sum()))}


def scissored_texels(width, height, guard_band):
    """Texels of the 16 layers outside the scissor guard_band / 4, from the sizes alone."""
    qw, qh, g = (width + 3) // 4, (height + 3) // 4, guard_band // 4
    return 16 * (qw * qh - max(0, qw - 2 * g) * max(0, qh - 2 * g))


def camera(width, height):
    from rsd.frame import FrameConfig, look_at
    return look_at([0.2, 2.1, 7.7], [0.1, 1.0, 0.0], [0.0, 1.0, 0.0],
                   FrameConfig(visible_w=width, visible_h=height, guard_band=0))


def tie_case(width=64, height=48):
    """An input whose taps fall exactly between two texels, where HLSL's round (half to even) and a round half
    away from zero part: a flat depth of 4, a Rand table of (1, 0, 0, 0) -- direction 0 is (1, 0) and RayPixels
    starts at 1 -- and a radius found by search (the shader's own float32 arithmetic, restated here) for which
    StepSizePixels is exactly 0.5, so direction 0 taps at 1, 1.5, 2 and 2.5 quarter texels.  The normals are the
    random ones of synthetic(), so the tap at 2 and the tap at 3 give different bytes.
    Returns dict(cam, layers, normal_w, rand, radius)."""
    cam, z = camera(width, height), F(4.0)
    sx, sy = F(0.5) * (F(cam.frameWidth) / F(cam.focalLength)), F(0.5) * (F(cam.frameHeight) / F(cam.focalLength))

    def step(r):
        a, b = (r / (sx * z) * F(0.5)) * F(width), (r / (sy * z) * F(0.5)) * F(height)
        return ((a + F(0.5) * (b - a)) / F(4.0)) / F(5.0)

    r = F(10.0) * F(2.0) * sy * z / F(height)
    candidates, down, up = [r], r, r
    for _ in range(64):
        down, up = np.nextafter(down, F(0)), np.nextafter(up, F(100))
        candidates += [down, up]
    radius = next(c for c in candidates if step(F(c)) == F(0.5))
    rand = np.tile(np.array([1.0, 0.0, 0.0, 0.0], F), (16, 1))
    s = synthetic(width, height)
    return dict(cam=cam, layers=np.full_like(s["layers"], z), normal_w=s["normal_w"], rand=rand, radius=float(radius))


def synthetic(width, height, zero_patch=16):
    """One synthetic frame: random linear depth in [2, 12] with smooth patches (two ramps and a stepped
    plateau, where the bright channel takes intermediate values), a patch at farZ, a patch of depth 0 in the
    top-left corner (the NaN taps: a texel there has P = 0 and an infinite radius in uv, whose lerp is NaN, so
    every tap's uv, S, VdotV and NdotV = 0 * inf or NaN are NaN and saturate turns them into no occlusion; 16
    pixels wide, so at guard band 8 half of it lies inside the scissor), random unit normals (about
    half of them facing away from the camera) and a second layer 0.05 to 3 behind the first.  zero_patch: the side
    of the depth-0 patch, for frames that 16 x 16 pixels would cover.
    Returns dict(cam, z, z2, normal_w, layers, layers2): full-size maps and their 16 layers."""
    rng = np.random.default_rng(width * 1000 + height)
    cam = camera(width, height)
    H, W = height, width
    z = (2.0 + 10.0 * rng.random((H, W))).astype(F)
    yy, xx = np.mgrid[0:H, 0:W].astype(F)
    h3, w3 = H // 3, W // 3
    z[h3:2 * h3, 0:w3] = (4.0 + 0.02 * xx + 0.03 * yy)[h3:2 * h3, 0:w3]              # a ramp
    z[2 * h3:H, w3:2 * w3] = (9.0 - 0.015 * xx + 0.01 * yy)[2 * h3:H, w3:2 * w3]     # a deeper one
    plateau = np.where((xx // 7 + yy // 5) % 2 == 0, F(3.0), F(3.4))                 # steps of 0.4
    z[0:h3, 2 * w3:W] = plateau[0:h3, 2 * w3:W]
    z[h3:h3 + H // 4, w3:w3 + W // 3] = F(cam.farZ)
    z[0:zero_patch, 0:zero_patch] = F(0.0)
    n = rng.normal(size=(H, W, 4)).astype(F)
    n[..., :3] /= np.linalg.norm(n[..., :3].astype(np.float64), axis=-1, keepdims=True).astype(F)
    z2 = (z + rng.uniform(0.05, 3.0, (H, W))).astype(F)
    out = dict(cam=cam, z=z, z2=z2, normal_w=np.ascontiguousarray(n), layers=deinterleave(z), layers2=deinterleave(z2))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
