"""CPU checks of the motion vectors of moving geometry (rsd_scene_track_motion, rsd_scene_motion_begin_frame,
rsd_gbuffer_motion): the brute-force checker the GPU tests compare against (tests/native/mvec_ref.c) is pinned to the
oracle's camera-only motion vectors, the definition satisfies the identity it must (moving the world by +v equals
moving the previous camera by +v) in float64, the float32 checker stays within its measured distance of the float64
evaluation, and the new C entries have the header's layout and refuse bad arguments without a GPU."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

import mvec_checker as MV
from conftest import ROOT
from helpers import to_oracle

needs_gcc = pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
SIZE = MV.SIZES[0]
SHIFT = (0.3, 0.1, -0.2)  # the camera's / the world's motion of these tests


@pytest.fixture(scope="module")
def checker(oracle, tmp_path_factory):
    return MV.build(oracle, tmp_path_factory.mktemp("mvec_ref"))


@pytest.fixture(scope="module")
def scenes():
    return {k: MV.make_scene(k) for k in MV.SCENES}


def _moved_cam(scene, size):
    c = scene.camera
    return MV.camera(scene, size, pos=[a + b for a, b in zip(c["pos"], SHIFT)])


@needs_gcc
@pytest.mark.parametrize("size", MV.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", list(MV.SCENES))
def test_projection_against_the_oracle(oracle, checker, scenes, kind, size):
    """prev_positions == positions and a moved camera: the checker's mvecW is +0 bits everywhere, and its mvec --
    projected from the hit itself -- agrees with oracle.motion_vectors_raster -- projected from the re-linearised
    raster depth of the oracle's own G-buffer -- to within half a pixel (0.5 / W, 0.5 / H): beyond that TemporalAO's
    tap would land on another texel.  Measured here (maximum |difference|, u / v), the same on arcade_tiny and
    foliage_small: 75 x 45 3.6e-07 / 3.6e-07 (half a pixel: 6.7e-03 / 1.1e-02), 13 x 7 3.0e-07 / 2.4e-07 (3.8e-02 /
    7.1e-02)."""
    W, H = size
    sc = scenes[kind]
    cur, prev = _moved_cam(sc, size), MV.camera(sc, size)
    got = MV.run(oracle, checker, sc, sc.positions, sc.positions, cur, prev, size, 1)
    assert not MV.bits(got["mvec_w"]).any(), "static geometry: mvecW is +0"
    osc = oracle.Scene(sc.positions, sc.indices, sc.flags, sc.alpha)
    oc, op = to_oracle(cur, oracle.Camera), to_oracle(prev, oracle.Camera)
    depth, _ = oracle.gbuffer_raster(osc, oc, W, H, 1)
    want = oracle.motion_vectors_raster(oc, op, depth)
    hit = got["prim"] != MV.MISS
    assert np.array_equal(hit, depth < 1.0) and hit.any()
    diff = np.abs(got["mvec"].astype(np.float64) - want.astype(np.float64))
    print(f"{kind} {W}x{H}: max |mvec - oracle| = {diff[..., 0].max():.3e} / {diff[..., 1].max():.3e} "
          f"(half a pixel {0.5 / W:.3e} / {0.5 / H:.3e})")
    assert diff[..., 0].max() <= 0.5 / W and diff[..., 1].max() <= 0.5 / H
    assert not MV.bits(got["mvec"][~hit]).any(), "a miss is (0, 0)"
    assert np.abs(got["mvec"][hit]).max() > 1e-3, "the camera moved: the vectors are not all zero"


@needs_gcc
@pytest.mark.parametrize("kind", list(MV.SCENES))
def test_moving_the_world_equals_moving_the_previous_camera(oracle, checker, scenes, kind):
    """The identity of the definition, in float64: every vertex moved by +v under a fixed camera (the previous
    positions are the positions - v) gives the motion vectors of the static scene whose previous camera stood at +v.
    Exact in real arithmetic; the two float64 evaluations differ by rounding alone (~1e-15 at these magnitudes), so
    they must agree to 1e-9."""
    sc = scenes[kind]
    cam = MV.camera(sc, SIZE)
    hits = MV.run(oracle, checker, sc, sc.positions, sc.positions, cam, cam, SIZE, 1)
    v = np.array(SHIFT, np.float64)
    pos = sc.positions.astype(np.float64)
    world, world_w = MV.mvec_f64(hits, sc.indices, pos, pos - v, cam, cam, SIZE)
    camera, camera_w = MV.mvec_f64(hits, sc.indices, pos, pos, cam, cam, SIZE, prev_cam_offset=v)
    hit = hits["prim"] != MV.MISS
    assert hit.any() and np.abs(world[hit]).max() > 1e-3
    d = np.abs(world - camera).max()
    print(f"{kind}: max |world - camera| = {d:.3e}")
    assert d <= 1e-9
    assert np.abs(world_w[hit] + v).max() <= 1e-12 and not camera_w.any()


# the largest |float32 checker - float64 evaluation| measured on the test scenes (test below), mvec and mvecW
MEASURED_MVEC, MEASURED_MVEC_W = 2.2e-07, 6.0e-08


@needs_gcc
@pytest.mark.parametrize("kind", list(MV.SCENES))
def test_float32_checker_against_float64(oracle, checker, scenes, kind):
    """The float32 checker against the float64 evaluation of the same formula from the same hits, positions and
    cameras, on moved geometry (P0 -> moved(1)) and a moved camera.  Measured (maximum absolute difference over the
    hit pixels in front of the previous camera): mvec arcade_tiny 2.10e-07, foliage_small 2.10e-07; mvecW
    arcade_tiny 4.21e-08, foliage_small 5.72e-08.  The records MEASURED_MVEC = 2.2e-07 and MEASURED_MVEC_W =
    6.0e-08 round these up; asserted with a 4x margin, which only guards against a different libm (sqrtf and the
    divisions are correctly rounded everywhere; the margin is for the compiler's choices in the oracle's library)."""
    sc = scenes[kind]
    cur, prev = _moved_cam(sc, SIZE), MV.camera(sc, SIZE)
    p1 = MV.moved(sc, 1)
    got = MV.run(oracle, checker, sc, p1, sc.positions, cur, prev, SIZE, 1)
    want, want_w = MV.mvec_f64(got, sc.indices, p1, sc.positions, cur, prev, SIZE)
    hit = got["prim"] != MV.MISS
    front = hit & (got["mvec"][..., 0] != 2.0)
    assert front.sum() > 0.5 * hit.sum() and MV.bits(got["mvec_w"])[hit].any()
    d = np.abs(got["mvec"][front].astype(np.float64) - want[front]).max()
    dw = np.abs(got["mvec_w"][hit][:, :3].astype(np.float64) - want_w[hit]).max()
    print(f"{kind}: max |f32 - f64| mvec {d:.3e}  mvecW {dw:.3e}")
    assert d <= 4 * MEASURED_MVEC and dw <= 4 * MEASURED_MVEC_W


@needs_gcc
def test_motion_info_layout(tmp_path):
    """sizeof(rsd_scene_motion_info) == 24 and its offsets, against the ctypes struct, through a compiled snippet."""
    from rsd import abi
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "rsd.h"\nint main(void){\n'
           'printf("%zu %zu %zu %zu %zu\\n", sizeof(rsd_scene_motion_info), offsetof(rsd_scene_motion_info, tracked),\n'
           'offsetof(rsd_scene_motion_info, reserved), offsetof(rsd_scene_motion_info, snapshots),\n'
           'offsetof(rsd_scene_motion_info, motion_bytes));\nreturn 0;}\n')
    (tmp_path / "s.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "s")], capture_output=True, text=True).stdout.split()]
    T = abi.SceneMotionInfo
    assert got == [24, 0, 4, 8, 16]
    assert got == [C.sizeof(T), T.tracked.offset, T.reserved.offset, T.snapshots.offset, T.motion_bytes.offset]
    assert C.sizeof(abi.SceneDynamicInfo) == 24 and C.sizeof(abi.SceneRigInfo) == 24  # no existing struct changed


def test_arguments_are_checked_without_a_gpu():
    """A null scene and null outputs get RSD_ERR_INVALID_ARG and a message naming the function, before any GPU work;
    the ABI version is unchanged."""
    from rsd import abi
    L = abi.lib()
    assert L.rsd_abi_version() == 8
    info = abi.SceneMotionInfo()
    assert L.rsd_scene_track_motion(None) == abi.ERR_INVALID_ARG and b"rsd_scene_track_motion" in L.rsd_last_error()
    assert L.rsd_scene_motion_begin_frame(None, None) == abi.ERR_INVALID_ARG
    assert b"rsd_scene_motion_begin_frame" in L.rsd_last_error()
    assert L.rsd_scene_motion_info_get(None, C.byref(info)) == abi.ERR_INVALID_ARG
    assert b"rsd_scene_motion_info_get" in L.rsd_last_error()
    d = C.c_void_p(16)  # never dereferenced: the checks come first
    assert L.rsd_scene_motion_info_get(d, None) == abi.ERR_INVALID_ARG
    cam = abi.Camera()
    ok = dict(scene=d, cam=C.byref(cam), prev=C.byref(cam), w=8, h=8, cull=1, depth=d, normal=d, mvec=d)

    def call(**kw):
        a = {**ok, **kw}
        return L.rsd_gbuffer_motion(a["scene"], a["cam"], a["prev"], a["w"], a["h"], a["cull"], a["depth"], a["normal"],
                                    None, a["mvec"], None, None)

    for bad in (dict(scene=None), dict(cam=None), dict(prev=None), dict(depth=None), dict(normal=None),
                dict(mvec=None), dict(w=0), dict(h=0), dict(cull=3)):
        assert call(**bad) == abi.ERR_INVALID_ARG, bad
        assert b"rsd_gbuffer_motion" in L.rsd_last_error(), bad


def test_header_declares_the_new_entries():
    from rsd import abi
    text = (ROOT / "include" / "rsd.h").read_text()
    for f in ("rsd_scene_track_motion", "rsd_scene_motion_begin_frame", "rsd_scene_motion_info_get",
              "rsd_gbuffer_motion"):
        assert f in abi.EXPORTS and f + "(" in text
