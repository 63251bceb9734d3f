"""The CPU checker of the AO-resolve tests (tests/native/ao_resolve_ref.c): a scalar restatement of the reference's
AOGuidedBlur and AOVarianceFix pixel shaders that shares no code with csrc/ao_resolve.hip, and the synthetic inputs
both test files run.  Shared by tests/test_ao_resolve.py (known answers, input conditions),
tests/test_gpu_ao_resolve.py and tests/test_gpu_graph_ao_resolve.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from hbao_checker import deinterleave, interleave  # noqa: F401  (DeinterleaveTexture / InterleaveTexture on the host)

HERE = Path(__file__).resolve().parent
F = np.float32
SENTINEL = 0x5A

# the counters of ao_resolve_ref.c
COUNTERS = ["tap_zero", "tap_half", "tap_clamped", "fallback_x", "fallback_y", "ldev_raised", "ldev_kept",
            "adev_raised", "adev_kept", "tie_out", "tie_ping", "means_fallback", "written"]
N_COUNTERS = 16
# the classes the issue names: every one of them is populated by the base inputs (tests/test_ao_resolve.py)
GUIDED_CLASSES = ["tap_zero", "tap_half", "tap_clamped", "fallback_x", "fallback_y", "ldev_raised", "ldev_kept", "tie_out"]
VARIANCE_CLASSES = ["tap_zero", "tap_half", "tap_clamped", "adev_raised", "adev_kept", "tie_out", "means_fallback"]

# (width, height, layers, guard band) of the full-size frame: 18 x 10 layers, a width that is no multiple of 4, scissor
# 8 / 4 = 2; 75-wide layers, two waves per row; one plain 9 x 9 image without a guard band; guard band 6, no multiple
# of 4 (scissor 1, uvMin and uvMax between texel centres)
CASES = [(70, 38, 16, 8), (300, 22, 16, 0), (9, 9, 1, 0), (70, 38, 16, 6)]
RADII = [1, 2, 4, 20]

_lib = None


def build(out_dir):
    """Compile the checker (once per process): gcc, no contraction, SSE arithmetic."""
    global _lib
    if _lib is None:
        so = Path(out_dir) / "libao_resolve_ref.so"
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-msse2", "-mfpmath=sse", "-shared", "-fPIC", "-o", str(so),
                        str(HERE / "native" / "ao_resolve_ref.c"), "-lm"], check=True)
        L = C.CDLL(str(so))
        vp, i = C.c_void_p, C.c_int
        L.ao_guided_blur_ref.restype = None
        L.ao_guided_blur_ref.argtypes = [vp, i, vp, i, i, i, i, i, i, i, i, vp, vp, vp]
        L.ao_variance_fix_ref.restype = None
        L.ao_variance_fix_ref.argtypes = [vp, vp, vp, i, i, i, i, i, i, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def layer_shape(width, height, layers):
    return (layers, (height + 3) // 4, (width + 3) // 4) if layers == 16 else (1, height, width)


def scissor(guard_band, layers):
    return guard_band // int(np.sqrt(float(layers)) + 0.5) if layers > 1 else guard_band


def inside(width, height, layers, guard_band):
    """Boolean mask [layers][qh][qw] of the texels inside the scissor."""
    L, qh, qw = layer_shape(width, height, layers)
    g = scissor(guard_band, layers)
    m = np.zeros((L, qh, qw), bool)
    if 2 * g < qw and 2 * g < qh:
        m[:, g:qh - g, g:qw - g] = True
    return m


def guided_blur(lib, src, depth, width, height, guard_band=0, radius=4, local_deviation=True, fill=SENTINEL):
    """(dst [L][qh][qw] uint8, pingpong [L][qh][qw][4] uint8, counters dict) of the checker.  src: [L][qh][qw][2] or
    [L][qh][qw] uint8 layers; depth: [L][qh][qw] float32; width, height: the full-size frame.  Texels outside the
    scissor keep `fill`."""
    src, z = np.ascontiguousarray(src, np.uint8), np.ascontiguousarray(depth, F)
    L, qh, qw = z.shape
    channels = 2 if src.ndim == 4 else 1
    assert src.shape[:3] == z.shape and z.shape == layer_shape(width, height, L) and (channels == 1 or src.shape[3] == 2)
    dst, ping = np.full((L, qh, qw), fill, np.uint8), np.full((L, qh, qw, 4), fill, np.uint8)
    counters = np.zeros(N_COUNTERS, np.uint64)
    lib.ao_guided_blur_ref(_p(src), channels, _p(z), qw, qh, L, width, height, int(guard_band), int(radius),
                           int(bool(local_deviation)), _p(ping), _p(dst), _p(counters))
    return dst, ping, dict(zip(COUNTERS, (int(v) for v in counters)))


def variance_fix(lib, bright, dark, depth, width, height, guard_band=0, fill=SENTINEL):
    """(dst [L][qh][qw] uint8, counters dict) of the checker; bright, dark: [L][qh][qw] uint8."""
    b, d, z = np.ascontiguousarray(bright, np.uint8), np.ascontiguousarray(dark, np.uint8), np.ascontiguousarray(depth, F)
    L, qh, qw = z.shape
    assert b.shape == z.shape and d.shape == z.shape and z.shape == layer_shape(width, height, L)
    dst, counters = np.full((L, qh, qw), fill, np.uint8), np.zeros(N_COUNTERS, np.uint64)
    lib.ao_variance_fix_ref(_p(b), _p(d), _p(z), qw, qh, L, width, height, int(guard_band), _p(dst), _p(counters))
    return dst, dict(zip(COUNTERS, (int(v) for v in counters)))


def synthetic(width, height, layers):
    """One synthetic frame, as layers.  Layer by layer, in layer texels (so that every layer has every feature):
      depth   4 + a ramp of 0.2 % per texel (depth weights near 1), the right third behind a step to twice the depth
              (weight exactly 0 across it, the two sides never mix), the lower rows with 3 % noise (weights in between),
              and a block of depth 0 whose texels take the weightSum fallback;
      bright  random in [90, 255], dark a random share of it, so ldev.y is above DARK_EPSILON there; the left columns
              hold constant bright and dark (ldev.y raised), one block has dark = 0 (AOVarianceFix's means fallback);
      ties    in the flat-depth band of rows 1 and 2, every texel of a column pair alternates between (a, b) and
              (a + 2 k, b + 2 k'): chosen so that some outputs land exactly between two bytes (asserted on the
              checker).
    Returns dict(ao2, bright, dark, depth): [L][qh][qw][2] / [L][qh][qw] uint8 and float32, read-only."""
    L, qh, qw = layer_shape(width, height, layers)
    rng = np.random.default_rng(width * 1000 + height * 10 + layers)
    yy, xx = np.mgrid[0:qh, 0:qw]
    z = np.empty((L, qh, qw), F)
    bright, dark = np.empty((L, qh, qw), np.uint8), np.empty((L, qh, qw), np.uint8)
    for s in range(L):
        d = (4.0 + 0.1 * s) * (1.0 + 0.002 * xx + 0.001 * yy)
        d = np.where(xx >= (2 * qw) // 3, 2.0 * d, d)
        noisy = yy >= (2 * qh) // 3
        d = np.where(noisy, d * (1.0 + rng.uniform(-0.03, 0.03, (qh, qw))), d)
        d[qh // 2:qh // 2 + 2, qw // 3:qw // 3 + 3] = 0.0
        z[s] = d.astype(F)
        b = rng.integers(90, 256, (qh, qw))
        k = (b * rng.uniform(0.2, 0.9, (qh, qw))).astype(np.int64)
        b[:, :max(2, qw // 6)] = 200 - s
        k[:, :max(2, qw // 6)] = 120 + s
        k[qh // 2 - 1:qh // 2 + 2, qw // 2:qw // 2 + 3] = 0
        bright[s], dark[s] = b.astype(np.uint8), k.astype(np.uint8)
    out = dict(bright=bright, dark=dark, depth=z, ao2=np.ascontiguousarray(np.stack([bright, dark], -1)))
    _tie_rows(out)
    for a in out.values():
        a.setflags(write=False)
    return out


def _tie_rows(s):
    """Rows 1 and 2 of every layer, between the constant columns and the depth step: bright alternates 100 / 140
    and dark 80 / 40 along x over a flat depth that doubles from row to row (no mixing in y), so the blurred means sit
    half way between the two values, both deviations are equal, w = (0.5, 0.5) and the output is the mean of a bright
    and a dark byte whose sum is odd for the (101, 40) texels."""
    L, qh, qw = s["depth"].shape
    x0, x1 = max(2, qw // 6), (2 * qw) // 3
    if qh < 4 or x1 - x0 < 3:
        return
    for row, scale in ((1, 1.0), (2, 2.0)):
        xs = np.arange(x0, x1)
        s["depth"][:, row, x0:x1] = F(3.0 * scale)
        s["bright"][:, row, x0:x1] = np.where(xs % 2 == 0, 101, 141)
        s["dark"][:, row, x0:x1] = np.where(xs % 2 == 0, 80, 40)
        s["ao2"][:, row, x0:x1, 0] = s["bright"][:, row, x0:x1]
        s["ao2"][:, row, x0:x1, 1] = s["dark"][:, row, x0:x1]
