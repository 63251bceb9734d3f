"""The brute-force any-hit reference and the stack model of the adversarial-geometry tests
(tests/native/hits_ref.c), with the cases they run on (tests/scenes_adversarial.py).  Shared by
tests/test_adversarial_walk.py (which pins the oracle to it) and tests/test_gpu_adversarial_walk.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import scenes_adversarial as SA

HERE = Path(__file__).resolve().parent
W, H = SA.W, SA.H
DEFAULT_DEPTH = np.float32(3.40282347e+37)  # the SD map's cleared value without normalisation
CAP = 48                                    # hits kept per texel (the counts go on beyond it)

_lib = None


def build(oracle, out_dir):
    """Compile the checker against the oracle's shared library (once per process)."""
    global _lib
    if _lib is None:
        olib = Path(oracle.build())
        so = Path(out_dir) / "libhits_ref.so"
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-I", str(olib.parents[1]),
                        "-o", str(so), str(HERE / "native" / "hits_ref.c"), str(olib),
                        f"-Wl,-rpath,{olib.parent}", "-lm"], check=True)
        oracle.lib()  # the oracle is loaded first: the checker binds to the same library
        L = C.CDLL(str(so))
        vp, u32 = C.c_void_p, C.c_uint32
        L.hits_ref.restype = None
        L.hits_ref.argtypes = [vp, C.c_int, vp, vp, vp, u32, vp, vp, vp, u32, u32, vp, vp, u32, u32, u32, vp, vp, vp,
                               vp, C.c_int]
        L.stack_model.restype = None
        L.stack_model.argtypes = [vp, u32, vp, u32, u32, u32, vp, vp, vp, C.c_int]
        _lib = L
    return _lib


class Case:
    """One adversarial scene with its oracle scene, the camera of the 65 x 49 frame and a zero depth input
    (TMin = 0.1 nearZ on every ray unless an interval map says otherwise)."""

    def __init__(self, oracle, name):
        from helpers import to_oracle
        from rsd.frame import make_camera
        self.name = name
        self.scene = SA.make(name)
        self.cfg = SA.frame_config()
        self.cam = make_camera(self.scene, self.cfg)
        self.ocam = to_oracle(self.cam, oracle.Camera)
        self.osc = oracle.Scene(self.scene.positions, self.scene.indices, self.scene.flags)
        self.has_alpha = False
        self.depth = np.zeros((H, W), np.float32)
        self.depth.setflags(write=False)
        self._hits = {}

    def sd_params(self, oracle, N=16, max_count=64, impl=3, cull=1, normalize=0, hit_order=0):
        """Jitter off, no guard band, ray intervals on (a zero word means no bound)."""
        return oracle.SDParams(N, impl, max_count, 0, 0, normalize, 1, cull, 1, float(np.float32(1.5 / N)), hit_order, 0)

    def hits(self, oracle, lib, cull=1, rmin=None, rmax=None):
        """(count [H, W], t, prim, t * cosT [H, W, CAP]) of every texel's ray; cached without interval maps."""
        key = cull if rmin is None and rmax is None else None
        if key is not None and key in self._hits:
            return self._hits[key]
        osc, sdp = self.osc, self.sd_params(oracle, cull=cull)
        cnt = np.zeros((H, W), np.uint32)
        t = np.zeros((H, W, CAP), np.float32)
        prim = np.zeros((H, W, CAP), np.uint32)
        zt = np.zeros((H, W, CAP), np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        lib.hits_ref(osc.h, 0, p(osc.positions), p(osc.indices), p(osc.flags), len(osc.indices), C.byref(self.ocam),
                     C.byref(sdp), p(self.depth), W, H, p(rmin), p(rmax), W, H, CAP, p(cnt), p(t), p(prim), p(zt),
                     oracle.effective_cpus())
        out = (cnt, t, prim, zt)
        if key is not None:
            for a in out:
                a.setflags(write=False)
            self._hits[key] = out
        return out


def first_depths(cnt, zt, n):
    """The K-buffer map the hit lists imply: the first n t * cosT per texel, DEFAULT_DEPTH beyond the count, in
    the SD map's layout [layer][y][x][channel]."""
    d = np.where(np.arange(n)[None, None, :] < cnt[..., None], zt[..., :n], DEFAULT_DEPTH).astype(np.float32)
    ch, layers = min(n, 4), (n + 3) // 4
    return np.ascontiguousarray(d.reshape(H, W, layers, ch).transpose(2, 0, 1, 3))


def stack_model(oracle, lib, case, bvh, tri_offset, cull=1):
    """(high-water mark, closest t, closest prim) [H, W] of the modelled depth-first walk of the primary rays
    over `bvh` (rsd.frame.host_bvh or GpuScene.export_bvh)."""
    b = np.ascontiguousarray(bvh, np.float32)
    mark = np.zeros((H, W), np.uint32)
    bt = np.zeros((H, W), np.float32)
    bp = np.zeros((H, W), np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.stack_model(p(b), int(tri_offset), C.byref(case.ocam), W, H, cull, p(mark), p(bt), p(bp), oracle.effective_cpus())
    return mark, bt, bp


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
