"""The CPU checker of the raster StochasticDepthMap tests (tests/native/sd_raster_ref.c): a brute-force
statement of rsd_sd_raster's semantics over the oracle's triangle test, alpha test, hash and stratified
table.  Shared by tests/test_sd_raster.py (which pins it to the oracle's G-buffers),
tests/test_gpu_sd_raster.py and tests/test_gpu_graph_sd_raster.py.

The frames are depth_peel_checker's: 75 x 45 pixels of the ~3000-triangle opaque and alpha scenes.  BASE
is the case the GPU tests vary around; its scene, camera, cull mode, sample count, Alpha and AO radius were
chosen on the CPU so that the checker alone meets BASE_MINIMUM (tests/test_sd_raster.py asserts it): every
discard rule, the stencil and the stratified masks act on at least 100 fragments or texels of that frame."""
import ctypes as C
import dataclasses
import subprocess
from pathlib import Path

import numpy as np

import depth_peel_checker as DP
from depth_peel_checker import SCENES, H, W, bits  # noqa: F401  (re-exported)

HERE = Path(__file__).resolve().parent

COUNTERS = ("fragments", "alpha", "first_layer", "ray_min", "ray_max", "r_zero", "stencilled", "two_values")
# The alpha scene seen from inside its corridor of foliage cards (several cards behind one another in most
# columns), no culling (the back faces of the props are fragments behind the first layer), AO radius 6 (pass
# 1 requests SD rays on a third of the 75 x 45 frame and leaves the rest stencilled out), and Alpha N = 0.8:
# a fragment covers one sample or none, so R == 0 occurs and texels with two survivors hold two values.
# Counters of this frame, from the checker alone: alpha 271, first_layer 1058, ray_min 122, ray_max 419,
# r_zero 138, stencilled 2317, two_values 118.
BASE = dict(kind="alpha", N=4, alpha=0.2, divisor=1, radius=6.0, cull=0)
BASE_CAMERA = dict(pos=[0.5, 1.3, 6.0], target=[0.0, 1.0, -8.0], up=[0.0, 1.0, 0.0])
BASE_MINIMUM = 100  # of each counter but "fragments" on the BASE frame with its intervals and stencil

_lib = None


class Case(DP.Case):
    """depth_peel_checker's case; the alpha scene is seen by BASE_CAMERA, the opaque one by its own camera."""

    def __init__(self, oracle, kind, size=(W, H)):
        super().__init__(oracle, kind, size)
        if kind == BASE["kind"]:
            from helpers import to_oracle
            from rsd.frame import look_at
            self.cam = look_at(BASE_CAMERA["pos"], BASE_CAMERA["target"], BASE_CAMERA["up"], self.cfg)
            self.ocam = to_oracle(self.cam, oracle.Camera)


class Params(C.Structure):  # sdr_params of sd_raster_ref.c = rsd_sd_raster_params
    _fields_ = [("sample_count", C.c_uint32), ("alpha", C.c_float), ("cull_mode", C.c_uint32),
                ("linearize", C.c_uint32), ("alpha_test", C.c_uint32), ("implementation", C.c_uint32),
                ("ray_interval", C.c_uint32), ("use_stencil", C.c_uint32)]


def params(N=4, alpha=None, cull=1, linearize=True, alpha_test=True, implementation=0, ray_interval=True,
           use_stencil=False):
    """alpha=None: SVAO's 1.5 / N (SVAO.cpp:164)."""
    a = float(np.float32(1.5 / N)) if alpha is None else float(alpha)
    return Params(N, a, cull, int(linearize), int(alpha_test), implementation, int(ray_interval), int(use_stencil))


def build(oracle, out_dir):
    """Compile the checker against the oracle's shared library (once per process)."""
    global _lib
    if _lib is None:
        olib = Path(oracle.build())
        so = Path(out_dir) / "libsd_raster_ref.so"
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-I", str(olib.parents[1]),
                        "-o", str(so), str(HERE / "native" / "sd_raster_ref.c"), str(olib),
                        f"-Wl,-rpath,{olib.parent}", "-lm"], check=True)
        oracle.lib()  # the oracle is loaded first: the checker binds to the same library
        L = C.CDLL(str(so))
        vp, u32 = C.c_void_p, C.c_uint32
        L.sd_raster_ref.restype = None
        L.sd_raster_ref.argtypes = [vp, C.c_int, vp, vp, vp, u32, vp, C.POINTER(Params), vp, u32, u32, vp, vp, vp, vp,
                                    u32, u32, vp, C.c_int]
        _lib = L
    return _lib


def raster(oracle, lib, case, prm, depth, sd_w, sd_h, rmin=None, rmax=None, stencil=None, ocam=None):
    """The checker's map, float32 [ceil(N / 4)][sd_h][sd_w][min(N, 4)], and its counters (a dict over
    COUNTERS).  depth: the non-linear first layer (any size); rmin / rmax: uint32 sd_h x sd_w or None;
    stencil: uint8 sd_h x sd_w or None."""
    N = prm.sample_count
    depth = np.ascontiguousarray(depth, np.float32)
    keep = [np.ascontiguousarray(a, t) if a is not None else None
            for a, t in ((rmin, np.uint32), (rmax, np.uint32), (stencil, np.uint8))]
    for a in keep:
        assert a is None or a.shape == (sd_h, sd_w)
    out = np.zeros(((N + 3) // 4, sd_h, sd_w, min(N, 4)), np.float32)
    cnt = np.zeros(8, np.uint64)
    osc = case.osc
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    lib.sd_raster_ref(osc.h, int(case.has_alpha), p(osc.positions), p(osc.indices), p(osc.flags), len(osc.indices),
                      C.byref(ocam if ocam is not None else case.ocam), C.byref(prm), p(depth), depth.shape[1],
                      depth.shape[0], p(keep[0]), p(keep[1]), p(keep[2]), p(out), sd_w, sd_h, p(cnt),
                      oracle.effective_cpus())
    return out, dict(zip(COUNTERS, (int(v) for v in cnt)))


def frame_config(divisor=1, radius=BASE["radius"], N=BASE["N"], cull=1, size=(W, H), **kw):
    """The frame of `size` (W x H by default) as SVAO's raster mode sees it: no guard bands, no SD jitter, exact
    numerics."""
    from rsd.frame import FrameConfig
    return FrameConfig(visible_w=size[0], visible_h=size[1], guard_band=0, divisor=divisor, sd_samples=N, sd_guard_px=0,
                       jitter=False, radius=radius, cull_mode=cull, numerics="exact", **kw)


@dataclasses.dataclass
class Frame:
    """The oracle's raster G-buffer of a case and its SVAO pass 1 (intervals and stencil of the SD map)."""
    cfg: object
    vao: object
    svp: object
    sd_w: int
    sd_h: int
    depth: np.ndarray      # non-linear, GBufferRaster.depth
    z: np.ndarray          # LinearizeDepth
    normals: np.ndarray    # CompressNormals
    ao1: np.ndarray
    stencil: np.ndarray
    rmin: np.ndarray
    rmax: np.ndarray


def oracle_frame(oracle, case, divisor=1, radius=BASE["radius"], N=BASE["N"], cull=1):
    from helpers import to_oracle
    from rsd.frame import make_vao, svao_params
    cfg = frame_config(divisor, radius, N, cull, size=case.size)
    vao, sd_w, sd_h = make_vao(cfg)
    ovao, svp = to_oracle(vao, oracle.VAOData), to_oracle(svao_params(cfg), oracle.SVAOParams)
    d, nw = oracle.gbuffer_raster(case.osc, case.ocam, case.size[0], case.size[1], cull)
    z = oracle.linearize_depth(d, case.ocam.nearZ, case.ocam.farZ)
    n = oracle.compress_normals(nw, case.ocam)
    ao1, st, rmin, rmax = oracle.svao_pass1(case.ocam, ovao, svp, z, n, sd_w, sd_h)
    for a in (d, z, n, ao1, st, rmin, rmax):
        a.setflags(write=False)
    return Frame(cfg, ovao, svp, sd_w, sd_h, d, z, n, ao1, st, rmin, rmax)
