"""The CPU checker of the post-AO image passes (tests/native/post_ref.c): a scalar restatement of the reference's
CrossBilateralBlur, TAA, Deinterleave / Interleave, RayMinMaxLength, AOFlickerMask, BinaryDilation and TemporalAO
shaders and of librsd's motion vectors that shares no code with csrc/post.hip or oracle/, an ImageEquation
evaluator of its own (formula text -> numpy float32), and the synthetic inputs of tests/test_post_checker.py
(known answers, input conditions) and tests/test_gpu_post_edges.py (GPU parity)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
F = np.float32
SENTINEL = 0xA5
PAD = 64  # texels of sentinel before and after every output buffer of the GPU tests

SIZES = [(1, 1), (3, 5), (63, 3), (64, 4), (65, 5), (129, 9)]  # (W, H): the edges of the 64 x 4 workgroup
# TemporalAO flag bits of post_ref.c
OUTSIDE, DEPTH_REJECT, STABLE, ACCUMULATED = 1, 2, 4, 8

_lib = None


def build(out_dir):
    """Compile the checker (once per process): gcc, no contraction, SSE arithmetic."""
    global _lib
    if _lib is None:
        so = Path(out_dir) / "libpost_ref.so"
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-msse2", "-mfpmath=sse", "-shared", "-fPIC", "-o", str(so),
                        str(HERE / "native" / "post_ref.c"), "-lm"], check=True)
        L = C.CDLL(str(so))
        vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
        sig = {"post_blur_weights": [vp, i32, i32, vp],
               "post_blur": [vp, i32, vp, i32, i32, vp, vp, i32, i32, i32, i32, i32],
               "post_catmull_rom_axis": [f32, f32, vp, vp],
               "post_taa": [vp, vp, vp, i32, i32, f32, f32, i32, vp],
               "post_deinterleave": [vp, i32, i32, i32, vp], "post_interleave": [vp, i32, i32, i32, vp],
               "post_ray_min_max_length": [vp, vp, i32, vp],
               "post_flicker_mask": [vp, vp, i32, i32, vp, f32, f32, f32, vp, vp, vp],
               "post_binary_dilation": [vp, i32, i32, i32, vp],
               "post_temporal_ao": [vp] * 7 + [i32, i32, i32, f32, f32, f32, vp, vp, vp, vp, vp],
               "post_motion_vectors": [vp, vp, vp, i32, i32, i32, vp, vp],
               "post_linear_axis": [f32, i32, vp, vp]}
        for name, args in sig.items():
            getattr(L, name).restype = None
            getattr(L, name).argtypes = args
        L.post_store_unorm8.restype, L.post_store_unorm8.argtypes = C.c_uint8, [f32]
        L.post_hlsl_min.restype, L.post_hlsl_min.argtypes = f32, [f32, f32]
        L.post_hlsl_max.restype, L.post_hlsl_max.argtypes = f32, [f32, f32]
        L.post_sample_unorm8_clamp.restype, L.post_sample_unorm8_clamp.argtypes = f32, [vp, i32, i32, f32, f32]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dt):
    return np.ascontiguousarray(a, dt)


# ------------------------------------------------------------------------------------------------ the operations

def blur_weights(lib, cache, better):
    cache = _c(cache, F)
    R = (cache.size - 1) // 2
    w = np.zeros(2 * R + 1, F)
    lib.post_blur_weights(_p(cache), R, int(better), _p(w))
    return w


def blur(lib, src, z, guard, radius, better, fill=SENTINEL):
    """src (H, W) or (H, W, texel) uint8, z (zh, zw) float32 -> (dst, pingpong), `fill` outside the scissor."""
    src, z = _c(src, np.uint8), _c(z, F)
    H, W = src.shape[:2]
    texel = 1 if src.ndim == 2 else src.shape[2]
    pp, dst = np.full((H, W), fill, np.uint8), np.full((H, W), fill, np.uint8)
    lib.post_blur(_p(src), texel, _p(z), z.shape[1], z.shape[0], _p(pp), _p(dst), W, H, guard, radius, int(better))
    return dst, pp


def catmull_rom_axis(lib, sample_pos, size):
    w, tc = np.zeros(4, F), np.zeros(3, F)
    lib.post_catmull_rom_axis(float(F(sample_pos)), float(size), _p(w), _p(tc))
    return w, tc


def taa(lib, color, mvec, prev, alpha=0.1, sigma=1.0, anti_flicker=True):
    color, mvec, prev = _c(color, F), _c(mvec, F), _c(prev, F)
    H, W = color.shape[:2]
    out = np.zeros((H, W, 4), F)
    lib.post_taa(_p(color), _p(mvec), _p(prev), W, H, alpha, sigma, int(bool(anti_flicker)), _p(out))
    return out


def deinterleave(lib, img):
    """(H, W[, c]) of any dtype -> (16, ceil(H/4), ceil(W/4)[, c])."""
    img = np.ascontiguousarray(img)
    H, W = img.shape[:2]
    texel = img.itemsize * int(np.prod(img.shape[2:], dtype=np.int64))
    out = np.full((16, (H + 3) // 4, (W + 3) // 4) + img.shape[2:], 0x7B, img.dtype)
    lib.post_deinterleave(_p(img), W, H, texel, _p(out))
    return out


def interleave(lib, layers, width, height):
    layers = np.ascontiguousarray(layers)
    texel = layers.itemsize * int(np.prod(layers.shape[3:], dtype=np.int64))
    out = np.zeros((height, width) + layers.shape[3:], layers.dtype)
    lib.post_interleave(_p(layers), width, height, texel, _p(out))
    return out


def ray_min_max_length(lib, rmin, rmax):
    rmin, rmax = _c(rmin, np.uint32), _c(rmax, np.uint32)
    out = np.zeros(rmin.shape, F)
    lib.post_ray_min_max_length(_p(rmin), _p(rmax), rmin.size, _p(out))
    return out


def flicker_mask(lib, z, normal_w, cam):
    """(mask, flags, dxy).  flags: 1 a neighbour outside the image, 2 a zero offset, 4 dx > 0.1, 8 dy > 0.1."""
    z, n = _c(z, F), _c(normal_w, F)
    H, W = z.shape
    view = np.array(list(cam.viewMat), F)
    mask, flags, dxy = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8), np.zeros((H, W, 2), F)
    lib.post_flicker_mask(_p(z), _p(n), W, H, _p(view), cam.frameWidth, cam.frameHeight, cam.focalLength, _p(mask),
                          _p(flags), _p(dxy))
    return mask, flags, dxy


def binary_dilation(lib, mask, op_max):
    mask = _c(mask, np.uint8)
    out = np.zeros_like(mask)
    lib.post_binary_dilation(_p(mask), mask.shape[1], mask.shape[0], int(op_max), _p(out))
    return out


def temporal_ao(lib, ao_in, z, mvec, prev_z, prev_ao, prev_n, stable, guard, cam, m, fill=SENTINEL):
    """(ao, history, flags, prev_depth): `fill` outside the scissor, flags / prev_depth 0 / NaN there."""
    ao_in, z, mvec, prev_z = _c(ao_in, np.uint8), _c(z, F), _c(mvec, F), _c(prev_z, F)
    prev_ao, prev_n = _c(prev_ao, np.uint8), _c(prev_n, np.uint8)
    stable = None if stable is None else _c(stable, np.uint8)
    H, W = z.shape
    m = _c(m, F).reshape(16)
    ao, n = np.full((H, W), fill, np.uint8), np.full((H, W), fill, np.uint8)
    flags, pd = np.zeros((H, W), np.uint8), np.full((H, W), np.nan, F)
    lib.post_temporal_ao(_p(ao_in), _p(z), _p(mvec), _p(prev_z), _p(prev_ao), _p(prev_n), _p(stable), W, H, guard,
                         cam.frameWidth, cam.frameHeight, cam.focalLength, _p(m), _p(ao), _p(n), _p(flags), _p(pd))
    return ao, n, flags, pd


def cam14(cam):
    return np.array(list(cam.posW) + list(cam.U) + list(cam.V) + list(cam.W) + [cam.nearZ, cam.farZ], F)


def motion_vectors(lib, cam, prev, z, raw=False):
    """(mvec (H, W, 2), pw |prev W| / |rel|: the cosine between the point and the previous view axis, NaN on the background)."""
    z = _c(z, F)
    H, W = z.shape
    out, ratio = np.zeros((H, W, 2), F), np.zeros((H, W), F)
    lib.post_motion_vectors(_p(cam14(cam)), _p(cam14(prev)), _p(z), int(raw), W, H, _p(out), _p(ratio))
    return out, ratio


def motion_vectors_double(cam, prev, z, raw=False):
    """The same projection in Python double, in its own order: the hit point from the unnormalised pixel ray
    (P = pos + z * dir / (dir . What)), then dot products with the previous axes over their squared lengths."""
    D = np.float64
    z = np.asarray(z, F).astype(D)
    H, W = z.shape
    if raw:
        n, f = D(F(cam.nearZ)), D(F(cam.farZ))
        z = n * f / (f + z * (n - f))
    u = ((np.arange(W, dtype=D) + 0.5) / W)[None, :]
    v = ((np.arange(H, dtype=D) + 0.5) / H)[:, None]
    U, V, Wv, pos = (np.array(list(a), D) for a in (cam.U, cam.V, cam.W, cam.posW))
    pU, pV, pW, ppos = (np.array(list(a), D) for a in (prev.U, prev.V, prev.W, prev.posW))
    d = (2 * u - 1)[..., None] * U + (1 - 2 * v)[..., None] * V + Wv
    P = pos + z[..., None] * d / (d @ (Wv / np.linalg.norm(Wv)))[..., None]
    rel = P - ppos
    pw = rel @ pW / (pW @ pW)
    with np.errstate(divide="ignore", invalid="ignore"):
        mx = (rel @ pU / (pU @ pU) / pw + 1) * 0.5 - u
        my = (1 - rel @ pV / (pV @ pV) / pw) * 0.5 - v
    return np.stack([mx, my], -1)


def cameras(width, height, near=0.1, far=1000.0):
    """The poses of the motion-vector tests: (current, [previous ...]): a translation, a rotation about the
    up axis, both, and a previous camera that looks back at the current one (every point behind it)."""
    from rsd.frame import FrameConfig, look_at
    cfg = FrameConfig(visible_w=width, visible_h=height, guard_band=0, near=near, far=far)
    up = [0.0, 1.0, 0.0]
    cur = look_at([0.2, 2.1, 7.7], [0.1, 1.0, 0.0], up, cfg)
    prevs = {"translation": look_at([0.5, 2.3, 8.2], [0.4, 1.2, 0.5], up, cfg),
             # small rotations: a 129 x 9 frame spans 83 degrees to either side, and the projection of a point near
             # 90 degrees from the previous view axis is ill-conditioned
             "rotation": look_at([0.2, 2.1, 7.7], [0.4, 1.05, 0.0], up, cfg),
             "both": look_at([0.0, 2.0, 8.1], [-0.2, 0.8, 0.0], up, cfg),
             "behind": look_at([0.2, 2.1, 7.0], [0.2, 2.3, 16.0], up, cfg)}
    return cur, prevs


# ------------------------------------------------------------------------------------------------ ImageEquation
# ImageEquation.ps.slang:8-13: float4 result = (FORMULA) over Texture2D<float4> I0..I3 read at xy.  librsd's rules:
# a scalar broadcasts, two vectors of different widths truncate to the narrower, exp2 / log2 / exp / log / sin / cos /
# rsqrt / pow in double rounded once (pow(x, 2) = x * x), min / max / clamp return the non-NaN operand.
R32F, RG32F, RGBA32F, R16U, R8U, R8UNORM, R32U, RG8UNORM = 0, 1, 2, 3, 4, 5, 6, 11
_TOKEN = re.compile(r"\s*(?:(\d+\.?\d*(?:[eE][-+]?\d+)?|\.\d+(?:[eE][-+]?\d+)?)[fFhH]?|([A-Za-z_]\w*)|(.))")
_DOUBLE1 = {"exp2": np.exp2, "log2": np.log2, "exp": np.exp, "log": np.log, "sin": np.sin, "cos": np.cos,
            "rsqrt": lambda d: 1.0 / np.sqrt(d)}


def float4_view(img, fmt, W, H):
    """What Texture2D<float4>[xy] reads over a W x H target: missing channels 0, alpha 1, 0 outside / unbound."""
    out = np.zeros((H, W, 4), F)
    if img is None:
        return out
    h, w = min(img.shape[0], H), min(img.shape[1], W)
    a = np.asarray(img)[:h, :w]
    t = out[:h, :w]
    t[..., 3] = 1
    if fmt == RGBA32F:
        t[...] = a
    elif fmt == RG32F:
        t[..., :2] = a
    elif fmt == RG8UNORM:
        t[..., :2] = a.astype(F) / F(255)
    elif fmt == R8UNORM:
        t[..., 0] = a.astype(F) / F(255)
    else:  # R32F and the three integer formats: the value itself
        t[..., 0] = a.astype(F)
    return out


class _Eval:
    """Recursive descent over the token list; every value is (three float32 arrays [H, W, 4], width): the result
    with every double transcendental nudged one double down, as computed, and one double up.  self.fragile marks the
    texels where a transcendental's three candidates did not round to one float."""

    def __init__(self, formula, views, W, H):
        self.toks = [(m.group(1), m.group(2), m.group(3)) for m in _TOKEN.finditer(formula) if m.group(0).strip()]
        self.i, self.views, self.shape = 0, views, (H, W, 4)
        self.fragile = np.zeros((H, W), bool)

    def peek(self):
        return self.toks[self.i][2] if self.i < len(self.toks) else None

    def sym(self, s):
        if self.peek() != s:
            raise ValueError(f"expected {s!r} at token {self.i}")
        self.i += 1

    @staticmethod
    def width(a, b):
        return b if a == 1 else a if b == 1 else min(a, b)

    def each(self, fn, *vals):
        return [fn(*(v[0][k] for v in vals)).astype(F) for k in range(3)]

    def double(self, fn, *vals):
        """fn in float64 on each variant, nudged by -1 / 0 / +1 double, each rounded to float32 once."""
        res = []
        for k in range(3):
            d = fn(*(v[0][k].astype(np.float64) for v in vals))
            if k != 1:
                d = np.nextafter(d, -np.inf if k == 0 else np.inf)
            res.append(d.astype(F))
        mid = fn(*(v[0][1].astype(np.float64) for v in vals))
        lo, hi = np.nextafter(mid, -np.inf).astype(F), np.nextafter(mid, np.inf).astype(F)
        m = mid.astype(F)
        differ = (lo.view(np.uint32) != m.view(np.uint32)) | (hi.view(np.uint32) != m.view(np.uint32))
        self.fragile |= (differ & ~np.isnan(m)).any(-1)
        return res

    def sum(self):
        v = self.product()
        while self.peek() in ("+", "-"):
            op = self.peek()
            self.i += 1
            r = self.product()
            v = (self.each((lambda a, b: a + b) if op == "+" else (lambda a, b: a - b), v, r), self.width(v[1], r[1]))
        return v

    def product(self):
        v = self.signed()
        while self.peek() in ("*", "/"):
            op = self.peek()
            self.i += 1
            r = self.signed()
            v = (self.each((lambda a, b: a * b) if op == "*" else (lambda a, b: a / b), v, r), self.width(v[1], r[1]))
        return v

    def signed(self):
        if self.peek() == "-":
            self.i += 1
            v = self.signed()
            return self.each(lambda a: -a, v), v[1]
        if self.peek() == "+":
            self.i += 1
            return self.signed()
        v = self.atom()
        while self.peek() == ".":
            self.i += 1
            name = self.toks[self.i][1]
            self.i += 1
            lanes = [("xyzw" if c in "xyzw" else "rgba").index(c) for c in name]
            if max(lanes) >= v[1]:
                raise ValueError("swizzle past the value's width")
            lanes = lanes + [lanes[0]] * (4 - len(lanes))
            v = ([a[..., lanes] for a in v[0]], len(name))
        return v

    def atom(self):
        num, ident, sym = self.toks[self.i]
        self.i += 1
        if num is not None:
            return [np.full(self.shape, F(float(num)), F)] * 3, 1
        if sym == "(":
            v = self.sum()
            self.sym(")")
            return v
        if ident is None:
            raise ValueError(f"unexpected {sym!r}")
        if re.fullmatch(r"I[0-3]", ident):
            self.sym("[")
            assert self.toks[self.i][1] == "xy"
            self.i += 1
            self.sym("]")
            return [self.views[int(ident[1])]] * 3, 4
        self.sym("(")
        args = [self.sum()]
        while self.peek() == ",":
            self.i += 1
            args.append(self.sum())
        self.sym(")")
        return self.call(ident, args)

    def call(self, name, args):
        w = args[0][1]
        for a in args[1:]:
            w = self.width(w, a[1])
        if name in ("float", "float2", "float3", "float4"):
            n = int(name[5:] or 1)
            if len(args) == 1 and args[0][1] == 1:
                return [np.repeat(a[..., :1], 4, -1) for a in args[0][0]], n
            out = []
            for k in range(3):
                lanes = np.concatenate([a[0][k][..., :a[1]] for a in args], -1)
                if lanes.shape[-1] != n:
                    raise ValueError("constructor widths do not add up")
                o = np.zeros(self.shape, F)
                o[..., :n] = lanes
                out.append(o)
            return out, n
        one = {"abs": np.abs, "sqrt": np.sqrt, "floor": np.floor, "ceil": np.ceil,
               "frac": lambda x: x - np.floor(x),
               "saturate": lambda x: np.fmin(np.fmax(x, F(0)), F(1)),  # NaN -> 0
               "sign": lambda x: (x > 0).astype(F) - (x < 0).astype(F)}
        if name in one:
            return self.each(one[name], args[0]), w
        if name in _DOUBLE1:
            return self.double(_DOUBLE1[name], args[0]), w
        if name == "min":
            return self.each(np.fmin, *args), w
        if name == "max":
            return self.each(np.fmax, *args), w
        if name == "step":  # step(y, x) = x >= y
            return self.each(lambda y, x: (x >= y).astype(F), *args), w
        if name == "pow":
            square = [b == F(2) for b in args[1][0]]
            general = self.double(np.power, *args)
            exact = [(a.astype(np.float64) * a.astype(np.float64)).astype(F) for a in args[0][0]]
            return [np.where(s, e, g) for s, e, g in zip(square, exact, general)], w
        if name == "lerp":  # x + s (y - x)
            return self.each(lambda x, y, s: x + s * (y - x), *args), w
        if name == "clamp":
            return self.each(lambda x, lo, hi: np.fmin(np.fmax(x, lo), hi), *args), w
        if name == "dot":
            def dot(a, b):
                p = a * b
                d = p[..., 0]
                for k in range(1, w):
                    d = d + p[..., k]
                return np.repeat(d[..., None], 4, -1)
            return self.each(dot, *args), 1
        raise ValueError(f"unknown function {name!r}")


def image_equation(formula, inputs, W, H):
    """inputs: four (image or None, format).  Returns (candidates [3][H, W, 4] float32, fragile [H, W] bool): the
    result as computed is candidates[1]."""
    views = [float4_view(img, fmt, W, H) for img, fmt in inputs]
    with np.errstate(all="ignore"):
        e = _Eval(formula, views, W, H)
        v, w = e.sum()
    if e.i != len(e.toks) or w not in (1, 4):
        raise ValueError("trailing tokens or a result that is neither a scalar nor a float4")
    return v, e.fragile


def store(lib, result, fmt):
    """The render-target write of a float4 result [H, W, 4]."""
    if fmt == RGBA32F:
        return result
    if fmt == RG32F:
        return np.ascontiguousarray(result[..., :2])
    if fmt == R32F:
        return np.ascontiguousarray(result[..., 0])
    x = np.ascontiguousarray(result[..., 0])
    return np.array([lib.post_store_unorm8(float(t)) for t in x.ravel()], np.uint8).reshape(x.shape)


def image_inputs(W, H, seed=0):
    """One image of each of the eight input formats: name -> (array, format).  Positive floats away from 0 in
    `rgba` and `rg` (log, rsqrt and pow stay finite), signed ones in `r32f`; `rg` is larger than the target and
    `r16` smaller, the rest of the target's size."""
    rng = np.random.default_rng(1000 * W + H + seed)
    return {"r8unorm": (rng.integers(0, 256, (H, W)).astype(np.uint8), R8UNORM),
            "rgba": ((0.05 + 3.0 * rng.random((H, W, 4))).astype(F), RGBA32F),
            "rg": ((0.05 + rng.random((H + 3, W + 5, 2))).astype(F), RG32F),
            "r32f": ((rng.random((H, W)) * 4 - 2).astype(F), R32F),
            "r8": (rng.integers(0, 256, (H, W)).astype(np.uint8), R8U),
            "r16": (rng.integers(0, 65536, (max(1, H - 1), max(1, W - 2))).astype(np.uint16), R16U),
            "r32": (rng.integers(0, 2 ** 32, (H, W), dtype=np.uint64).astype(np.uint32), R32U),
            "rg8": (rng.integers(0, 256, (H, W, 2)).astype(np.uint8), RG8UNORM)}


# (formula, the four inputs by name): every input format, every F1 / F2 / F3 function, dot of 2, 3 and 4 lanes
EQUATIONS = [
    ("I0[xy].r + I1[xy].r / 255.0 + I2[xy].r / 65535.0 + I3[xy].r / 4294967296.0", ("r8unorm", "r8", "r16", "r32")),
    ("float4(I0[xy].rg, I1[xy].gr)", ("rg8", "rg", None, None)),                       # ExtractBright / ExtractDark read rg8
    ("I0[xy].g", ("rg8", None, None, None)),
    ("exp(-I0[xy]) + log(I0[xy]) * rsqrt(I0[xy].wzyx)", ("rgba", None, None, None)),
    ("exp2(I1[xy].r) - log2(I0[xy]) + sin(I1[xy].r * 3.0) * cos(I0[xy])", ("rgba", "r32f", None, None)),
    ("floor(I0[xy] * 3.0) + ceil(I1[xy].r * 3.0) * sign(I1[xy].r) + sign(I0[xy] - 1.5) + frac(I0[xy] * 7.0)",
     ("rgba", "r32f", None, None)),
    ("abs(I1[xy].r) + saturate(I0[xy] - 1.0) + sqrt(I0[xy]) * step(0.5, I1[xy].r)", ("rgba", "r32f", None, None)),
    ("min(I0[xy], I1[xy].rgrg) + max(I0[xy].wzyx, 1.0) + pow(I0[xy], 2.2) + pow(I0[xy], 2.0)", ("rgba", "rg", None, None)),
    ("lerp(I0[xy], I0[xy].wzyx, I1[xy].r) + clamp(I0[xy], 0.5, I1[xy].g + 1.0)", ("rgba", "rg", None, None)),
    ("dot(I0[xy].xy, I1[xy].xy) + dot(I0[xy].xyz, I0[xy].zyx) * dot(I0[xy], I0[xy].wzyx)", ("rgba", "rg", None, None)),
    # six pending left operands and the two of the innermost operation: eight values on the stack
    ("I0[xy] - (I0[xy].wzyx + (I1[xy].r / (2.0 - (I0[xy].yxwz * (I1[xy].g + (3.0 - I0[xy]))))))",
     ("rgba", "rg", None, None)),
]
DEPTH8 = EQUATIONS[-1][0]
DEPTH9 = "I0[xy] - (0.5 * (I0[xy].wzyx + (I1[xy].r / (2.0 - (I0[xy].yxwz * (I1[xy].g + (3.0 - I0[xy])))))))"


def unorm_formula(formula):
    """The formula folded into [0, 1) for an R8Unorm target: most of EQUATIONS exceed 1 and would store 255."""
    return f"frac(({formula}) * 0.173)"


# ------------------------------------------------------------------------------------------------ synthetic inputs

def ray_case(W, H):
    """(rayMin, rayMax) words: random intervals, a fifth never raised (rayMax == 0), some inverted, and the special
    bit patterns +-inf, NaN, the smallest denormal and -0 in every pairing (as far as the frame has room)."""
    rng = np.random.default_rng(W * 19 + H)
    mn = (rng.random((H, W)) * 50).astype(F)
    mx = (mn + (rng.random((H, W)) * 10 - 2)).astype(F)
    mnu, mxu = mn.view(np.uint32).copy(), mx.view(np.uint32).copy()
    mxu[rng.random((H, W)) < 0.2] = 0
    special = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0x00000001, 0x80000000], np.uint32)
    k = min(25, W * H)
    mnu.reshape(-1)[:k] = np.repeat(special, 5)[:k]
    mxu.reshape(-1)[:k] = np.tile(special, 5)[:k]
    return mnu, mxu


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def largest_guard(W, H):
    """The largest guard band that leaves a scissor one pixel wide or high."""
    return (min(W, H) - 1) // 2


def blur_case(W, H, texel=1, z_scale=(1, 1)):
    """A random R8Unorm (texel 1) or RG8Unorm (texel 2) image and a depth of (H * zs_y // zd_y, W * ...) texels: a
    smooth ramp with noise, a depth edge, and single texels of 0, +inf and NaN."""
    rng = np.random.default_rng(W * 131 + H * 7 + texel)
    num, den = z_scale
    zw, zh = max(1, W * num // den), max(1, H * num // den)
    yy, xx = np.mgrid[0:zh, 0:zw].astype(F)
    z = (5.0 + 0.11 * xx + 0.07 * yy + 0.05 * rng.random((zh, zw)) + (xx > 0.6 * zw) * 20.0).astype(F)
    if zw >= 9 and zh >= 3:
        for k, bad in enumerate((0.0, np.inf, np.nan)):
            z[zh // 2, 2 + 3 * k] = bad      # each is the centre tap of its own texel and a side tap of its neighbours
            z[(zh // 2 + 1) % zh, zw - 3 - 3 * k] = bad
    src = rng.integers(0, 256, (H, W) if texel == 1 else (H, W, texel)).astype(np.uint8)
    return _freeze(dict(src=src, z=z))


def _reach(base, target):
    """A float32 m with base + m == target (in float32), searched within a few ulps of target - base; (m, found)."""
    base, target = np.asarray(base, F), np.broadcast_to(np.asarray(target, F), np.shape(base))
    m = (target - base).astype(F)
    found = (base + m).astype(F) == target
    for step in (1, -1, 2, -2, 3, -3):
        c = m.copy()
        for _ in range(abs(step)):
            c = np.nextafter(c, F(np.inf) if step > 0 else F(-np.inf))
        ok = ~found & ((base + c).astype(F) == target)
        m = np.where(ok, c, m)
        found |= ok
    return m, found


TAO_CATEGORIES = (["default"] * 6 + [f"{lim}_{side}" for lim in ("minx", "maxx", "miny", "maxy")
                                     for side in ("below", "on", "above")]
                  + ["ratio_in", "ratio_out", "depth0", "prev_depth0", "n0", "n29", "n30", "n255", "tie", "centre"])


def tao_matrix():
    """prevViewToCurView of a small camera move: a rotation of 0.02 about y and a translation, row-major."""
    c, s = np.cos(0.02), np.sin(0.02)
    return np.array([[c, 0, s, 0.05], [0, 1, 0, -0.02], [-s, 0, c, 0.11], [0, 0, 0, 1]], F)


def tao_case(lib, W, H, guard, use_mask, cam):
    """TemporalAO inputs whose scissor texels cycle through TAO_CATEGORIES (dict `cat`: name -> boolean image of
    the texels where the construction succeeded).  The reprojected uv of the limit categories is built from the
    shader's own float32 sum texC + mvec; the depth categories from the checker's reprojected depth."""
    rng = np.random.default_rng(W * 977 + H * 31 + guard * 3 + int(use_mask))
    m = tao_matrix()
    g = guard
    ao = rng.integers(0, 256, (H, W)).astype(np.uint8)
    prev_ao = rng.integers(0, 256, (H, W)).astype(np.uint8)
    prev_n = rng.integers(0, 31, (H, W)).astype(np.uint8)
    prev_z = (2.0 + 10.0 * rng.random((H, W))).astype(F)
    mv = rng.normal(0.0, 0.6 / max(W, 8), (H, W, 2)).astype(F)
    mv[rng.random((H, W)) < 0.08] = 0.7
    idx = np.full((H, W), -1)
    sh, sw = H - 2 * g, W - 2 * g
    idx[g:H - g, g:W - g] = (np.arange(sh * sw).reshape(sh, sw) * 5 + 3) % len(TAO_CATEGORIES)
    # texC + mvec reaches a float next to a small limit only where mvec is small too (its own rounding step is
    # that of the larger operand): the lower limits get the first columns and rows of the scissor as well
    names = list(TAO_CATEGORIES)
    yy, xx = np.mgrid[0:H, 0:W]
    if sw >= 12 and sh >= 3:
        rows = (yy >= g) & (yy < g + (2 if sh >= 9 else 1)) & (xx >= g) & (xx < W - g)
        idx[rows] = (names.index("miny_below") + xx % 3)[rows]
        cols = (xx >= g) & (xx < g + 4) & (yy >= g) & (yy < H - g)
        idx[cols] = (names.index("minx_below") + (xx + yy) % 3)[cols]
    cat = {name: np.zeros((H, W), bool) for name in set(TAO_CATEGORIES)}
    for k, name in enumerate(TAO_CATEGORIES):
        cat[name] |= idx == k
    tu = ((np.arange(W, dtype=F) + F(0.5)) / F(W))[None, :].repeat(H, 0)
    tv = ((np.arange(H, dtype=F) + F(0.5)) / F(H))[:, None].repeat(W, 1)
    lim = {"minx": (F(g) + F(0.5)) / F(W), "maxx": (F(W) - (F(g) + F(0.5))) / F(W),
           "miny": (F(g) + F(0.5)) / F(H), "maxy": (F(H) - (F(g) + F(0.5))) / F(H)}   # GuardBand.cpp:62-63
    special = idx >= 6
    mv[special] = 0.0
    prev_n[special] = 5
    for name, t in lim.items():
        axis, base = (0, tu) if name.endswith("x") else (1, tv)
        for side, target in (("below", np.nextafter(t, F(-1))), ("on", t), ("above", np.nextafter(t, F(2)))):
            sel = cat[f"{name}_{side}"]
            mm, found = _reach(base, target)
            mv[..., axis] = np.where(sel & found, mm, mv[..., axis])
            cat[f"{name}_{side}"] = sel & found
    # bilinear fractions of the previous AO: sample position p = i + k / 256 + 1 / 512 (a tie) or p = i (a centre)
    for name, frac in (("tie", lambda k: F(k) / F(256) + F(1.0 / 512)), ("centre", lambda k: F(0) * F(k))):
        sel = cat[name]
        ys, xs = np.nonzero(sel)
        for y, x in zip(ys, xs):
            ok = True
            for axis, n, i, base in ((0, W, x, tu[y, x]), (1, H, y, tv[y, x])):
                fr = frac((3 * x + 5 * y) % 256)
                pi = min(max(i + (1 if (x + y) % 2 else -1), g), n - 1 - g)
                if fr > 0 and pi == n - 1 - g:   # stay inside the valid area
                    pi -= 1
                if pi < g:
                    ok = False
                    break
                p = F(pi) + fr
                u0, hit = F((p + F(0.5)) / F(n)), None
                for c in [u0] + [np.nextafter(u0, F(s)) for s in (-1, 2)]:
                    if F(F(c * F(n)) - F(0.5)) == p:
                        hit = c
                        break
                if hit is None:
                    ok = False
                    break
                mm, found = _reach(F(base), hit)
                ok &= bool(found)
                mv[y, x, axis] = mm
            if not ok:
                mv[y, x] = 0.0
                cat[name][y, x] = False
    prev_n[cat["n0"]], prev_n[cat["n29"]], prev_n[cat["n30"]], prev_n[cat["n255"]] = 0, 29, 30, 255
    if W * H >= 40:
        prev_z[rng.random((H, W)) < 0.02] = 0.0
    prev_z[cat["prev_depth0"]] = 0.0
    # the reprojected depth of every texel inside the valid area (it does not depend on the current depth)
    _, _, _, pd = temporal_ao(lib, ao, np.ones((H, W), F), mv, prev_z, prev_ao, prev_n, None, guard, cam, m)
    pd = np.where(np.isnan(pd), F(5.0), pd)
    z = np.where(special, pd, pd * (1.0 + rng.uniform(-0.2, 0.2, (H, W)))).astype(F)
    # |1 - prevDepth / depth| next to 0.1: depth near prevDepth / 0.9, the quotient near 0.9 has steps of 2^-24, so
    # the test value takes the multiples of 2^-24 nearest to 0.1 on either side
    cand = (pd / F(0.9)).astype(F)
    best_in, best_out = np.full((H, W), np.nan, F), np.full((H, W), np.nan, F)
    rel_in, rel_out = np.full((H, W), -np.inf, F), np.full((H, W), np.inf, F)
    c = cand.copy()
    for _ in range(12):
        c = np.nextafter(c, F(-np.inf))
    with np.errstate(all="ignore"):
        for _ in range(25):
            rel = np.abs(F(1.0) - pd / c).astype(F)
            better_in = (rel < F(0.1)) & (rel > rel_in)
            better_out = (rel >= F(0.1)) & (rel < rel_out)
            best_in, rel_in = np.where(better_in, c, best_in), np.where(better_in, rel, rel_in)
            best_out, rel_out = np.where(better_out, c, best_out), np.where(better_out, rel, rel_out)
            c = np.nextafter(c, F(np.inf))
    close = F(2.0 ** -23)
    cat["ratio_in"] &= (F(0.1) - rel_in) <= close
    cat["ratio_out"] &= (rel_out - F(0.1)) <= close
    z = np.where(cat["ratio_in"], best_in, z)
    z = np.where(cat["ratio_out"], best_out, z)
    z[cat["depth0"]] = 0.0
    mask = None
    if use_mask:
        mask = ((rng.random((H, W)) < 0.2) & ~special).astype(np.uint8)
    return _freeze(dict(ao=ao, z=z.astype(F), mv=mv, prev_z=prev_z, prev_ao=prev_ao, prev_n=prev_n, mask=mask, m=m,
                        cat=cat, limits=lim, tu=tu, tv=tv))


TAA_JUMPS = [0.6, -0.6, 1.3, -1.3, 7.25, -7.25]
TAA_KINDS = ["small", "centre", "tie"] + [f"jump{j:+g}" for j in TAA_JUMPS]


def taa_selected_motion(mv):
    """TAA.ps.slang:121-127 on the host: the motion vector each texel samples with, the longest of its 3 x 3
    neighbourhood in the shader's order (the texel's own first; a later one only if strictly longer; 0 outside)."""
    H, W = mv.shape[:2]
    pad = np.zeros((H + 2, W + 2, 2), F)
    pad[1:-1, 1:-1] = mv
    sel = mv.copy()
    best = (sel[..., 0] * sel[..., 0] + sel[..., 1] * sel[..., 1]).astype(F)
    for dx, dy in ((-1, -1), (-1, 1), (1, -1), (1, 1), (1, 0), (0, -1), (0, 1), (-1, 0)):
        m = pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        l2 = (m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]).astype(F)
        take = l2 > best
        sel = np.where(take[..., None], m, sel)
        best = np.where(take, l2, best)
    return sel


def catmull_rom_centre_tap(tc, mv, n):
    """TAA.ps.slang:48-61 along one axis in numpy float32 (arrays): the fraction f of the sample position and the
    position, in texels, at which the linear sampler reads the centre tap tc12 (uv * size - 0.5)."""
    n = F(n)
    sp = ((tc + mv).astype(F) * n).astype(F)
    c = (np.floor(sp - F(0.5)) + F(0.5)).astype(F)
    f = (sp - c).astype(F)
    f2 = f * f
    f3 = f2 * f
    w0 = f2 - F(0.5) * (f3 + f)
    w1 = F(1.5) * f3 - F(2.5) * f2 + F(1)
    w3 = F(0.5) * (f3 - f2)
    w2 = F(1) - w0 - w1 - w3
    tc12 = (c + w2 / (w1 + w2)) * (F(1) / n)
    return f, (tc12 * n - F(0.5)).astype(F)


def on_tie(p):
    """A sample position whose fraction is k / 256 + 1 / 512 exactly."""
    t = (p - np.floor(p)).astype(F) * F(256)
    return (t - np.floor(t)) == F(0.5)


def taa_classify(c):
    """name -> boolean image: the kind of the motion each texel of a taa_case actually samples with."""
    sel = taa_selected_motion(c["mv"])
    H, W = sel.shape[:2]
    tu = ((np.arange(W, dtype=F) + F(0.5)) / F(W))[None, :].repeat(H, 0)
    tv = ((np.arange(H, dtype=F) + F(0.5)) / F(H))[:, None].repeat(W, 1)
    fx, px = catmull_rom_centre_tap(tu, sel[..., 0], W)
    fy, py = catmull_rom_centre_tap(tv, sel[..., 1], H)
    texels = np.hypot(sel[..., 0].astype(np.float64) * W, sel[..., 1].astype(np.float64) * H)
    out = {f"jump{j:+g}": (sel[..., 0] == F(j)) & (sel[..., 1] == F(-j / 2)) for j in TAA_JUMPS}
    moved = texels >= 1.0
    out["centre"] = (fx == 0) & (fy == 0) & moved & (texels < 8)
    out["tie"] = on_tie(px) & on_tie(py) & moved
    out["small"] = (texels > 0) & (texels < 3) & ~out["centre"] & ~out["tie"]
    return out


def _tie_motion(rng, tc, n):
    """A motion of 2 to 4 images along one axis that puts the centre tap of texel coordinate tc on a tie, found
    among 2^15 random candidates with the shader's float32 arithmetic (far from the origin the sample position
    has few fraction bits, so about one candidate in 2^9 .. 2^12 is a tie); None if there is none."""
    cand = rng.uniform(2.0, 4.0, 1 << 15).astype(F)
    _, p = catmull_rom_centre_tap(np.full(cand.shape, tc, F), cand, n)
    hit = np.nonzero(on_tie(p))[0]
    return cand[hit[0]] if hit.size else None


def taa_case(W, H, first_frame=False):
    """Random colours in [0, 2), a random history (zeros on a first frame) and finite motion, laid out in column
    bands of one kind each so that the longest vector of a 3 x 3 neighbourhood (the one the shader samples with)
    is of the band's kind: small random vectors; a uniform shift of (2, -1) texels, which lands the sample on a
    texel centre wherever the float32 (texC + motion) * texDim is exact; single texels between zero-motion
    neighbours whose vector puts the Catmull-Rom centre tap c + w2 / w12 on a k/256 + 1/512 tie in both axes (the
    outer taps c - 1 and c + 2 are always texel centres); uniform jumps of +-0.6, +-1.3 and +-7.25 images (wrap
    through several periods and negative indices).  Frames narrower than 18 columns cycle the kinds by rows."""
    rng = np.random.default_rng(W * 613 + H * 17)
    color = (rng.random((H, W, 4)) * 2).astype(F)
    prev = np.zeros((H, W, 4), F) if first_frame else (rng.random((H, W, 4)) * 2).astype(F)
    nk = len(TAA_KINDS)
    yy, xx = np.mgrid[0:H, 0:W]
    band = (xx * nk // W) if W >= 2 * nk else (yy % nk if H > 1 else np.zeros((H, W), int))
    mv = np.zeros((H, W, 2), F)
    small = band == 0
    mv[small] = rng.normal(0.0, 0.7 / max(W, 8), (int(small.sum()), 2)).astype(F)
    mv[band == 1] = (F(2) / F(W), F(-1) / F(H))
    for k, j in enumerate(TAA_JUMPS):
        mv[band == 3 + k] = (j, -j / 2)
    cells = (band == 2) & (xx % 3 == 1) & ((yy % 3 == 1) | (H < 3))
    for y, x in zip(*np.nonzero(cells)):
        mx = _tie_motion(rng, (F(x) + F(0.5)) / F(W), W)
        my = _tie_motion(rng, (F(y) + F(0.5)) / F(H), H)
        if mx is not None and my is not None:
            mv[y, x] = (mx, my)
    return _freeze(dict(color=color, prev=prev, mv=mv))


FLICKER_WINDOW = F(1e-6)   # one float step of the tilt moves |dot| by about 3e-8, the normalisations by 1e-7


def _tilted_normals(cam, t):
    """World-space unit normals whose view-space direction is the view axis tilted by t towards view x."""
    view = np.array(list(cam.viewMat), F).reshape(4, 4)
    v = view[2, :3] * (F(1) - t[..., None]) + view[0, :3] * t[..., None]
    return (v / np.linalg.norm(v.astype(np.float64), axis=-1, keepdims=True)).astype(F)


def flicker_case(lib, W, H):
    """A depth map with a slope, a step and noise, a block of depth 0 (every view position there is the origin, so
    the offsets between neighbours are zero vectors and normalize gives NaN), and normals: random ones on a third
    of the texels; on the rest the view axis tilted towards view x by a per-texel amount found by bisection on the
    checker's own dx, so that dx = min |dot| sits within FLICKER_WINDOW of 0.1, on alternate texels at or below it
    and above it (`near_in`, `near_out`: where the bisection closed and dy stays below the threshold, so the mask
    follows dx)."""
    from rsd.frame import FrameConfig, look_at
    rng = np.random.default_rng(W * 71 + H)
    cam = look_at([0.3, 2.0, 8.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0], FrameConfig(visible_w=max(W, 2), visible_h=max(H, 2),
                                                                                  guard_band=0))
    yy, xx = np.mgrid[0:H, 0:W]
    z = (4.0 + 0.01 * xx + 0.02 * yy + rng.normal(0, 0.002, (H, W))).astype(F)
    z[:, W // 2:] += F(1.5)
    if W >= 8 and H >= 4:
        z[1:H - 1, 2:min(W // 3, 24)] = 0.0
    n = rng.normal(0, 1, (H, W, 4)).astype(F)
    n[..., :3] /= np.linalg.norm(n[..., :3].astype(np.float64), axis=-1, keepdims=True).astype(F)
    random_normal = (xx + 2 * yy) % 3 == 0

    def dxy_of(t):
        nn = n.copy()
        nn[..., :3] = np.where(random_normal[..., None], n[..., :3], _tilted_normals(cam, t))
        return nn, flicker_mask(lib, z, nn, cam)[2]

    lo, hi = np.zeros((H, W), F), np.full((H, W), 0.6, F)
    with np.errstate(invalid="ignore"):
        bracket = (dxy_of(lo)[1][..., 0] <= F(0.1)) & (dxy_of(hi)[1][..., 0] > F(0.1))
        for _ in range(40):
            mid = ((lo + hi) * F(0.5)).astype(F)
            below = dxy_of(mid)[1][..., 0] <= F(0.1)
            lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
        want_in = (xx + yy) % 2 == 0
        normal_w, dxy = dxy_of(np.where(want_in, lo, hi))
        close = bracket & ~random_normal & (np.abs(dxy[..., 0] - F(0.1)) <= FLICKER_WINDOW) & (dxy[..., 1] <= F(0.1))
    return _freeze(dict(cam=cam, z=z, normal_w=np.ascontiguousarray(normal_w), near_in=close & want_in & (dxy[..., 0] <= F(0.1)),
                        near_out=close & ~want_in & (dxy[..., 0] > F(0.1))))
