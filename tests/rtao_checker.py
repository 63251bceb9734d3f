"""The CPU checker of the RTAO tests (tests/native/rtao_ref.c): a brute-force statement of rsd_rtao's rays and of
rsd_gbuffer_world's positions over the oracle's triangle test and alpha test, with its own MT19937, sample table
and hash.  Shared by tests/test_rtao.py and tests/test_gpu_rtao.py; the float64 restatements of the sample table
and of Falcor's UniformSampleGenerator live here too (numpy only)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import depth_peel_checker as DP

HERE = Path(__file__).resolve().parent
W, H = DP.W, DP.H  # 75 x 45: partial 8x8 tiles on both axes
SCENES = DP.SCENES
Case = DP.Case
bits = DP.bits
SAMPLES = 5312
TMIN = np.float32(0.001)

_lib = None


def build(oracle, out_dir):
    """Compile the checker against the oracle's shared library (once per process)."""
    global _lib
    if _lib is None:
        olib = Path(oracle.build())
        so = Path(out_dir) / "librtao_ref.so"
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-I", str(olib.parents[1]),
                        "-o", str(so), str(HERE / "native" / "rtao_ref.c"), str(olib),
                        f"-Wl,-rpath,{olib.parent}", "-lm"], check=True)
        oracle.lib()  # the oracle is loaded first: the checker binds to the same library
        L = C.CDLL(str(so))
        vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
        for name, res, args in [
            ("rtao_mt_ref", None, [u32, u32, vp]),
            ("rtao_table_ref", None, [vp]),
            ("rtao_jenkins_ref", u32, [u32]),
            ("rtao_hash_ref", u32, [u32, u32, u32]),
            ("rtao_origins_ref", None, [vp, vp, u32, f32, vp]),
            ("rtao_dirs_ref", None, [vp, vp, u32, u32, u32, u32, vp]),
            ("rtao_trace_ref", None, [vp, C.c_int, vp, vp, vp, u32, vp, vp, u32, u32, f32, f32, vp, C.c_int]),
            ("rtao_posw_ref", None, [vp, C.c_int, vp, vp, vp, u32, vp, u32, u32, u32, vp]),
        ]:
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a, shape):
    a = np.ascontiguousarray(a, np.float32)
    assert a.shape == shape, (a.shape, shape)
    return a


def mt_raw(lib, seed, n):
    out = np.zeros(n, np.uint32)
    lib.rtao_mt_ref(seed, n, _p(out))
    return out


def table(lib):
    out = np.zeros(SAMPLES, np.uint32)
    lib.rtao_table_ref(_p(out))
    return out


def posw(oracle, lib, case, cull, has_alpha=None, ocam=None, width=W, height=H):
    osc = case.osc
    out = np.zeros((height, width, 4), np.float32)
    lib.rtao_posw_ref(osc.h, int(case.has_alpha if has_alpha is None else has_alpha), _p(osc.positions),
                      _p(osc.indices), _p(osc.flags), len(osc.indices), C.byref(ocam if ocam is not None else case.ocam),
                      width, height, cull, _p(out))
    return out


def origins(lib, pos_w, face_n, normal_scale):
    h, w = pos_w.shape[:2]
    pos_w, face_n = _f32(pos_w, (h, w, 4)), _f32(face_n, (h, w, 4))
    out = np.zeros((h, w, 4), np.float32)
    lib.rtao_origins_ref(_p(pos_w), _p(face_n), h * w, float(normal_scale), _p(out))
    return out


def dirs(lib, pos_w, face_n, frame, index_shift=0):
    """The spp = 1 directions (h x w x 4, w = 0)."""
    h, w = pos_w.shape[:2]
    pos_w, face_n = _f32(pos_w, (h, w, 4)), _f32(face_n, (h, w, 4))
    out = np.zeros((h, w, 4), np.float32)
    lib.rtao_dirs_ref(_p(pos_w), _p(face_n), w, h, int(frame), int(index_shift), _p(out))
    return out


def trace(oracle, lib, osc, has_alpha, orig, d, tmax, tmin=TMIN):
    """t per ray (0 = miss): orig h x w x 4, d h x w x spp x 4 (or h x w x 4 for spp = 1)."""
    h, w = orig.shape[:2]
    orig = _f32(orig, (h, w, 4))
    d = np.ascontiguousarray(d, np.float32).reshape(h, w, -1, 4)
    spp = d.shape[2]
    out = np.zeros((h, w, spp), np.float32)
    lib.rtao_trace_ref(osc.h, int(has_alpha), _p(osc.positions), _p(osc.indices), _p(osc.flags), len(osc.indices),
                       _p(orig), _p(d), h * w, spp, float(tmin), float(tmax), _p(out), oracle.effective_cpus())
    return out


# ---- float32 / float64 restatements in numpy
def ambient_no_falloff(t, min_ambient):
    """CalculateAO without the exponential falloff, in float32: a hit gives 1 - (1 - minAmbient) * 1."""
    one = np.float32(1.0)
    return np.where(t > 0, one - (one - np.float32(min_ambient)) * one, one).astype(np.float32)


def ray_distance(t, tmax):
    """The pass's rayDistance from the per-ray t (h x w x spp, 0 = miss) in float32: one ray gives its distance;
    more give (maxAORayTHit + the sum of the distances in ray order) / spp -- the reference's sum starts at
    maxAORayTHit."""
    tmax = np.float32(tmax)
    d = np.where(t > 0, t, tmax).astype(np.float32)
    spp = t.shape[-1]
    if spp == 1:
        return d[..., 0]
    acc = np.full(t.shape[:-1], tmax, np.float32)
    for i in range(spp):
        acc = (acc + d[..., i]).astype(np.float32)
    return (acc / np.float32(spp)).astype(np.float32)


def jenkins(a):
    a = np.asarray(a, np.uint32).copy()
    with np.errstate(over="ignore"):
        a -= a << np.uint32(6)
        a ^= a >> np.uint32(17)
        a -= a << np.uint32(9)
        a ^= a << np.uint32(4)
        a -= a << np.uint32(3)
        a ^= a << np.uint32(10)
        a ^= a >> np.uint32(15)
    return a


def pixel_hash(x, y, frame):
    with np.errstate(over="ignore"):
        return jenkins(np.asarray(x, np.uint32) * np.uint32(449) + np.asarray(y, np.uint32) * np.uint32(2857) +
                       jenkins(np.uint32(frame)))


def table_float64():
    """The sample table's components before rounding, in float64: (5312 x 3) values v * 127 from
    numpy.random.MT19937 seeded like std::mt19937(89)."""
    g = np.random.MT19937()
    g._legacy_seeding(89)
    raw = g.random_raw(2 * SAMPLES).astype(np.uint32)
    u = (raw.astype(np.float32) * np.float32(2.0 ** -32)).astype(np.float32)
    u = np.where(u >= 1, np.nextafter(np.float32(1), np.float32(0)), u).astype(np.float64).reshape(SAMPLES, 2)
    phi = u[:, 1] * 2.0 * np.pi
    t = np.sqrt(1.0 - u[:, 0])
    s = np.sqrt(1.0 - t * t)
    return np.stack([s * np.cos(phi), s * np.sin(phi), t], -1) * 127.0


def _spread16(v):
    v = np.asarray(v, np.uint32) & np.uint32(0xffff)
    v = (v | (v << np.uint32(8))) & np.uint32(0x00ff00ff)
    v = (v | (v << np.uint32(4))) & np.uint32(0x0f0f0f0f)
    v = (v | (v << np.uint32(2))) & np.uint32(0x33333333)
    v = (v | (v << np.uint32(1))) & np.uint32(0x55555555)
    return v


def interleave_32bit(x, y):
    return _spread16(x) | (_spread16(y) << np.uint32(1))


def _splitmix64(state):
    with np.errstate(over="ignore"):
        state = state + np.uint64(0x9E3779B97F4A7C15)
        z = state
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return state, z ^ (z >> np.uint64(31))


def _rotl(x, k):
    return (x << np.uint32(k)) | (x >> np.uint32(32 - k))


def uniform_generator(x, y, sample_number, n):
    """n successive next() values (n x shape, uint32) of Falcor's UniformSampleGenerator(pixel, sampleNumber)."""
    x, y = np.asarray(x, np.uint32), np.asarray(y, np.uint32)
    st = (np.uint64(sample_number) << np.uint64(32)) | interleave_32bit(x, y).astype(np.uint64)
    st, a = _splitmix64(st)
    st, b = _splitmix64(st)
    m = np.uint64(0xffffffff)
    s = [(a & m).astype(np.uint32), (a >> np.uint64(32)).astype(np.uint32), (b & m).astype(np.uint32),
         (b >> np.uint64(32)).astype(np.uint32)]
    out = []
    with np.errstate(over="ignore"):
        for _ in range(n):
            out.append(_rotl(s[0] * np.uint32(5), 7) * np.uint32(9))
            t = s[1] << np.uint32(9)
            s[2] = s[2] ^ s[0]
            s[3] = s[3] ^ s[1]
            s[1] = s[1] ^ s[2]
            s[0] = s[0] ^ s[3]
            s[2] = s[2] ^ t
            s[3] = _rotl(s[3], 11)
    return np.stack(out)


def dirs_float64(face_n, frame, spp):
    """The spp > 1 directions in float64 (h x w x spp x 3): UniformSampleGenerator(pixel, frame), sampleNext2D per
    ray, sample_cosine_hemisphere_polar, the pass's tangent frame of the float32 face normal."""
    h, w = face_n.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    r = uniform_generator(xx, yy, frame, 2 * spp)
    u = (r >> np.uint32(8)).astype(np.float64) * 2.0 ** -24  # h x w each
    f = face_n[..., :3].astype(np.float64)
    with np.errstate(invalid="ignore"):  # a pixel the G-buffer missed has no normal (and no ray)
        n = f / np.linalg.norm(f, axis=-1, keepdims=True)
    zero = np.zeros_like(n[..., 0])
    b = np.where((np.abs(n[..., 0]) > np.abs(n[..., 1]))[..., None],
                 np.stack([-n[..., 2], zero, n[..., 0]], -1), np.stack([zero, n[..., 2], -n[..., 1]], -1))
    t = np.cross(b, n)
    out = np.zeros((h, w, spp, 3))
    for i in range(spp):
        ux, uy = u[2 * i], u[2 * i + 1]
        rr, phi = np.sqrt(ux), 2.0 * np.pi * uy
        s = np.stack([rr * np.cos(phi), rr * np.sin(phi), np.sqrt(1.0 - ux)], -1)
        v = t * s[..., 0:1] + b * s[..., 1:2] + n * s[..., 2:3]
        with np.errstate(invalid="ignore"):
            out[:, :, i] = v / np.linalg.norm(v, axis=-1, keepdims=True)
    return out
