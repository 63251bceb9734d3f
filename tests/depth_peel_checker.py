"""The CPU checker of the DepthPeeling tests (tests/native/depth_peel_ref.c): a brute-force statement of
rsd_depth_peel's semantics over the oracle's triangle test and alpha test.  Shared by
tests/test_depth_peel.py (which pins it to the oracle's G-buffers) and tests/test_gpu_depth_peel.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
W, H = 75, 45  # partial 8x8 tiles on both axes
SCENES = {"opaque": ("arcade_tiny", 3000), "alpha": ("foliage_small", 3000)}

_lib = None


def build(oracle, out_dir):
    """Compile the checker against the oracle's shared library (once per process)."""
    global _lib
    if _lib is None:
        olib = Path(oracle.build())
        so = Path(out_dir) / "libdepth_peel_ref.so"
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-I", str(olib.parents[1]),
                        "-o", str(so), str(HERE / "native" / "depth_peel_ref.c"), str(olib),
                        f"-Wl,-rpath,{olib.parent}", "-lm"], check=True)
        oracle.lib()  # the oracle is loaded first: the checker binds to the same library
        L = C.CDLL(str(so))
        vp, u32 = C.c_void_p, C.c_uint32
        L.depth_peel_ref.restype = None
        L.depth_peel_ref.argtypes = [vp, C.c_int, vp, vp, vp, u32, vp, u32, u32, u32, vp, C.c_float, u32, vp, C.c_int]
        _lib = L
    return _lib


class Case:
    """One small scene with its oracle scene and the camera of a frame of `size` (width, height), W x H by default."""

    def __init__(self, oracle, kind, size=(W, H)):
        from rsd.frame import FrameConfig, make_camera
        from rsd.scenes import make_scene
        name, tris = SCENES[kind]
        self.scene = make_scene(name, target_tris=tris)
        self.size = tuple(size)
        self.cfg = FrameConfig(visible_w=size[0], visible_h=size[1], guard_band=0)
        self.cam = make_camera(self.scene, self.cfg)
        from helpers import to_oracle
        self.ocam = to_oracle(self.cam, oracle.Camera)
        self.osc = oracle.Scene(self.scene.positions, self.scene.indices, self.scene.flags, self.scene.alpha)
        self.has_alpha = self.scene.alpha is not None


def peel(oracle, lib, case, cull, prev, min_separation, linear_out, ocam=None, width=W, height=H):
    """The checker's layer behind `prev` (float32 height x width): raster depth or linear depth."""
    prev = np.ascontiguousarray(prev, np.float32)
    assert prev.shape == (height, width)
    out = np.zeros((height, width), np.float32)
    osc = case.osc
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.depth_peel_ref(osc.h, int(case.has_alpha), p(osc.positions), p(osc.indices), p(osc.flags),
                       len(osc.indices), C.byref(ocam if ocam is not None else case.ocam), width, height, cull,
                       p(prev), float(min_separation), int(linear_out), p(out), oracle.effective_cpus())
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
