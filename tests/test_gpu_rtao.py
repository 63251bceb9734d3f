"""GPU: rsd_gbuffer_world, rsd_rtao, the RTAO graph pass and Renderer.rtao against the brute-force CPU checker
(tests/native/rtao_ref.c).  75 x 45 frames of ~3000-triangle scenes: partial 8 x 8 tiles on both axes.  Ray
directions of spp = 1, hit parameters, ray distances and the ambient term without falloff are compared bitwise;
what goes through sin / cos / exp by the bounds stated at each test.

Mutants of csrc/rtao.hip and what catches them (each test first shows that its frame is sensitive to the mutation,
with the checker alone):
  TMin dropped                      test_normal_scale_zero (the checker with tmin = 0 differs on that frame)
  alpha test skipped                test_alpha_scene (the checker without alpha data differs)
  frame_index ignored               test_one_sample_matches_the_checker (frames 0, 1, 7 differ from each other)
  table index off by one            test_one_sample_matches_the_checker (the checker with the shifted index differs)
  maxAORayTHit seed of the sum gone test_four_samples (the sum without the seed differs)
  wrong generator seed or order     test_four_samples (directions off by ~0.1 against the 1e-5 bound)
  a hit farther than the closest    test_adversarial_scenes (40 layers 3 ulps apart, 10 coincident triangles)
The (t, prim) tie-break itself cannot show in RTAO's outputs: they are functions of the closest t alone, and
triangles that tie in t give the same t whichever wins.  test_adversarial_scenes pins what is observable: the
exact minimum among exact and near ties (and says where a BVH walk and a brute force may differ: shear_ties)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import rtao_checker as RT
import scenes_adversarial as ADV
from conftest import ROOT

pytestmark = pytest.mark.gpu

W, H = RT.W, RT.H
SCRIPT = ROOT / "tests" / "graphs" / "rtao.py"
MAX_T = 12.0    # of a 40 x 12 x 40 room: about a fifth of the rays hit
CLIP_FAR = 18.0  # the median depth of the frames: the clipped camera's G-buffer misses about half the pixels
bits = RT.bits


@pytest.fixture(scope="session")
def checker(oracle, tmp_path_factory):
    return RT.build(oracle, tmp_path_factory.mktemp("rtao_ref"))


class Gpu:
    """The two small scenes on the GPU and their world G-buffers (computed once, never modified)."""

    def __init__(self, oracle):
        import torch
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from rsd import abi
        from rsd.frame import Device, GpuScene
        self.torch, self.abi, self.oracle = torch, abi, oracle
        self.dev = Device(0)
        self.cases = {k: RT.Case(oracle, k) for k in RT.SCENES}
        self.scenes = {k: GpuScene(self.dev, c.scene) for k, c in self.cases.items()}
        self._gb = {}

    def camera(self, kind, clipped):
        """(librsd camera, oracle camera): the case's, or the same with farZ pulled in to CLIP_FAR."""
        c = self.cases[kind]
        cam, ocam = self.abi.Camera.from_buffer_copy(c.cam), self.oracle.Camera.from_buffer_copy(c.ocam)
        if clipped:
            cam.farZ = ocam.farZ = CLIP_FAR
        return cam, ocam

    def empty(self, shape, dtype=None):
        t = self.torch
        return t.full(shape, -7.0, dtype=dtype or t.float32, device="cuda")

    def gbuffer_world(self, kind, clipped, cull=1):
        """(depth, faceNormalW, posW) of rsd_gbuffer_world as read-only numpy arrays."""
        key = (kind, clipped, cull)
        if key not in self._gb:
            abi, p = self.abi, lambda x: C.c_void_p(x.data_ptr())
            cam, _ = self.camera(kind, clipped)
            d, nw, pw = self.empty((H, W)), self.empty((H, W, 4)), self.empty((H, W, 4))
            abi.check(abi.lib().rsd_gbuffer_world(self.scenes[kind].h, C.byref(cam), W, H, cull, p(d), p(nw), p(pw),
                                                  None), "rsd_gbuffer_world")
            self.torch.cuda.synchronize()
            out = tuple(x.cpu().numpy() for x in (d, nw, pw))
            for a in out:
                a.setflags(write=False)
            self._gb[key] = out
        return self._gb[key]

    def rtao(self, scene_handle, pos_w, face_n, prm, frame=0):
        """rsd_rtao on the given G-buffer: (ambient, ray_distance, ray log h x w x spp x 4) as numpy."""
        t, abi, p = self.torch, self.abi, lambda x: C.c_void_p(x.data_ptr())
        h, w = pos_w.shape[:2]
        pw, fn = t.from_numpy(np.array(pos_w, np.float32)).cuda(), t.from_numpy(np.array(face_n, np.float32)).cuda()
        amb, dist, log = self.empty((h, w)), self.empty((h, w)), self.empty((h, w, prm.spp, 4))
        abi.check(abi.lib().rsd_rtao(scene_handle, C.byref(prm), w, h, p(pw), p(fn), frame, p(amb), p(dist), p(log),
                                     None), "rsd_rtao")
        t.cuda.synchronize()
        return amb.cpu().numpy(), dist.cpu().numpy(), log.cpu().numpy()

    def t_max(self, prm):
        v = C.c_float()
        self.abi.check(self.abi.lib().rsd_rtao_ray_t_max(C.byref(prm), C.byref(v)), "rsd_rtao_ray_t_max")
        return np.float32(v.value)

    def close(self):
        for s in self.scenes.values():
            s.release()
        self.dev.close()


@pytest.fixture(scope="module")
def gpu(oracle):
    g = Gpu(oracle)
    yield g
    g.close()


def params(gpu, **kw):
    kw.setdefault("max_t_hit", MAX_T)
    kw.setdefault("apply_exponential_falloff", False)
    return gpu.abi.RTAOParams(**kw)


def expect_one_sample(oracle, checker, osc, has_alpha, pos_w, face_n, prm, tmax, frame):
    """The checker's frame of spp = 1 without falloff: (ambient, ray_distance, ray log)."""
    orig = RT.origins(checker, pos_w, face_n, prm.normal_scale)
    d = RT.dirs(checker, pos_w, face_n, frame)
    t = RT.trace(oracle, checker, osc, has_alpha, orig, d, tmax)
    log = np.concatenate([d[..., None, :3], t[..., None]], -1)
    return RT.ambient_no_falloff(t[..., 0], prm.minimum_ambient_illumination), RT.ray_distance(t, tmax), log


def assert_frame_equal(got, want):
    for g, w, name in zip(got, want, ("ambient", "ray_distance", "ray log")):
        np.testing.assert_array_equal(bits(g), bits(w), err_msg=name)


@pytest.mark.parametrize("kind", ["opaque", "alpha"])
@pytest.mark.parametrize("clipped", [False, True])
def test_world_gbuffer(oracle, checker, gpu, kind, clipped):
    """Depth and normal are rsd_gbuffer_raster's bits; posW is the checker's (o + d t, 1), 0 on a miss."""
    t, abi, p = gpu.torch, gpu.abi, lambda x: C.c_void_p(x.data_ptr())
    cam, ocam = gpu.camera(kind, clipped)
    d, nw, pw = gpu.gbuffer_world(kind, clipped)
    d0, nw0 = gpu.empty((H, W)), gpu.empty((H, W, 4))
    abi.check(abi.lib().rsd_gbuffer_raster(gpu.scenes[kind].h, C.byref(cam), W, H, 1, p(d0), p(nw0), None),
              "rsd_gbuffer_raster")
    t.cuda.synchronize()
    np.testing.assert_array_equal(bits(d), bits(d0.cpu().numpy()))
    np.testing.assert_array_equal(bits(nw), bits(nw0.cpu().numpy()))
    want = RT.posw(oracle, checker, gpu.cases[kind], 1, ocam=ocam)
    np.testing.assert_array_equal(bits(pw), bits(want))
    hit = pw[..., 3] == 1.0
    assert (hit == (d < 1.0)).all() and (pw[~hit] == 0).all()
    if clipped:
        assert hit.mean() >= 0.05 and (~hit).mean() >= 0.05


def test_one_sample_matches_the_checker(oracle, checker, gpu):
    """spp = 1 without falloff at frame indices 0, 1 and 7, on a G-buffer with hit and miss pixels: ray_distance,
    ambient and the logged rays are the checker's bits; the frames differ; a table index off by one would show."""
    c = gpu.cases["opaque"]
    _, nw, pw = gpu.gbuffer_world("opaque", True)
    prm = params(gpu)
    tmax = gpu.t_max(prm)
    assert tmax == np.float32(MAX_T)
    frames = {}
    for frame in (0, 1, 7):
        got = gpu.rtao(gpu.scenes["opaque"].h, pw, nw, prm, frame)
        want = expect_one_sample(oracle, checker, c.osc, c.has_alpha, pw, nw, prm, tmax, frame)
        assert_frame_equal(got, want)
        frames[frame] = got
    amb, dist, log = frames[0]
    valid = pw[..., 3] != 0
    hit = log[..., 0, 3] > 0
    assert (hit & valid).sum() >= 0.05 * valid.sum() and (~hit & valid).sum() >= 0.05 * valid.sum()
    assert (amb[~valid] == 1).all() and (dist[~valid] == tmax).all() and (log[~valid] == 0).all()
    assert (amb[hit] == np.float32(1) - (np.float32(1) - np.float32(0.07))).all() and (amb[~hit] == 1).all()
    for a, b in ((0, 1), (0, 7), (1, 7)):
        assert (bits(frames[a][2]) != bits(frames[b][2]))[valid].any(axis=(-1, -2)).mean() > 0.9
        assert (bits(frames[a][1]) != bits(frames[b][1])).any()
    shifted = RT.dirs(checker, pw, nw, 0, index_shift=1)
    assert (bits(shifted[..., :3]) != bits(log[..., 0, :3]))[valid].any(axis=-1).mean() > 0.9


@pytest.fixture(scope="module")
def four(gpu):
    """spp = 4 with the default falloff at frame 3 on the clipped opaque G-buffer (shared by two tests)."""
    _, nw, pw = gpu.gbuffer_world("opaque", True)
    prm = params(gpu, spp=4, apply_exponential_falloff=True)
    return dict(prm=prm, frame=3, out=gpu.rtao(gpu.scenes["opaque"].h, pw, nw, prm, 3), tmax=gpu.t_max(prm), nw=nw, pw=pw)


def test_four_samples(oracle, checker, gpu, four):
    """spp = 4: the logged directions are the float64 restatement of the generator within 1e-5 per component (about
    80 ulp of sin / cos and rounding; a wrong seed or index is off by ~0.1), the logged t is the checker's trace of
    the logged directions bit for bit, and ray_distance is (maxAORayTHit + sum of the distances) / 4 bit for bit."""
    c = gpu.cases["opaque"]
    amb, dist, log = four["out"]
    nw, pw, tmax = four["nw"], four["pw"], four["tmax"]
    valid = pw[..., 3] != 0
    want_d = RT.dirs_float64(nw, four["frame"], 4)
    err = np.abs(log[..., :3].astype(np.float64) - want_d)[valid]
    print("spp 4: max direction error", err.max())
    assert err.max() <= 1e-5
    assert (log[~valid] == 0).all()
    orig = RT.origins(checker, pw, nw, four["prm"].normal_scale)
    dirs4 = np.concatenate([log[..., :3], np.zeros_like(log[..., :1])], -1)
    t = RT.trace(oracle, checker, c.osc, c.has_alpha, orig, dirs4, tmax)
    np.testing.assert_array_equal(bits(log[..., 3]), bits(t))
    hits = (t > 0)[valid]
    assert hits.mean() >= 0.05 and (~hits).mean() >= 0.05
    want = RT.ray_distance(t, tmax)
    want[~valid] = tmax
    np.testing.assert_array_equal(bits(dist), bits(want))
    # the reference's sum starts at maxAORayTHit: without that seed the frame would differ
    d = np.where(t > 0, t, tmax).astype(np.float32)
    plain = ((((d[..., 0] + d[..., 1]).astype(np.float32) + d[..., 2]).astype(np.float32) + d[..., 3]).astype(np.float32)
             / np.float32(4)).astype(np.float32)
    assert (bits(plain) != bits(dist))[valid].all()
    # the four rays of a pixel differ from each other and from the next frame's
    assert (np.abs(log[..., 0, :3] - log[..., 1, :3]).max(-1) > 1e-3)[valid].mean() > 0.99
    again = gpu.rtao(gpu.scenes["opaque"].h, pw, nw, four["prm"], four["frame"] + 1)[2]
    assert (np.abs(again[..., :3] - log[..., :3]).max(-1) > 1e-3)[valid].mean() > 0.99


@pytest.mark.parametrize("spp", [1, 4])
def test_falloff(oracle, checker, gpu, four, spp):
    """Exponential falloff on: |ambient - the float64 formula on the logged t| <= 1e-6 (two 1-ulp exp
    implementations, at most 6e-8 each below 1, plus spp roundings of the mean)."""
    if spp == 4:
        prm, tmax, (amb, dist, log), pw = four["prm"], four["tmax"], four["out"], four["pw"]
    else:
        _, nw, pw = gpu.gbuffer_world("opaque", True)
        prm = params(gpu, apply_exponential_falloff=True)
        tmax = gpu.t_max(prm)
        amb, dist, log = gpu.rtao(gpu.scenes["opaque"].h, pw, nw, prm, 5)
    # RTAO.cpp:134-141: the traced length is sqrt(ln(cutoff) / -lambda) maxTHit
    cutoff, lam = np.float64(np.float32(prm.min_occlusion_cutoff)), np.float64(prm.exponential_falloff_decay_constant)
    assert abs(tmax - np.sqrt(np.log(cutoff) / -lam) * MAX_T) <= 1e-6 * MAX_T
    t = log[..., 3].astype(np.float64)
    assert (t <= tmax).all() and (t > 0).any()
    occ = np.exp(-lam * (t / np.float64(prm.max_t_hit)) ** 2)
    per_ray = np.where(t > 0, 1.0 - (1.0 - np.float64(np.float32(prm.minimum_ambient_illumination))) * occ, 1.0)
    want = per_ray.mean(-1)
    err = np.abs(amb.astype(np.float64) - want)
    print(f"spp {spp}: max ambient error", err.max())
    assert err.max() <= 1e-6
    valid = pw[..., 3] != 0
    assert (amb[~valid] == 1).all() and (dist[~valid] == tmax).all()
    hit = (t > 0).any(-1)
    assert (amb[hit] < 1).all() and len(np.unique(amb[hit])) > 10  # the falloff grades the hits


def test_alpha_scene(oracle, checker, gpu):
    """Alpha-tested cards: the frame is the checker's with the alpha test, and differs from the same geometry
    uploaded without its alpha data, which is the checker's without the test."""
    from rsd.frame import GpuScene
    c = gpu.cases["alpha"]
    assert c.has_alpha
    _, nw, pw = gpu.gbuffer_world("alpha", False)
    prm = params(gpu)
    tmax = gpu.t_max(prm)
    got = gpu.rtao(gpu.scenes["alpha"].h, pw, nw, prm, 2)
    assert_frame_equal(got, expect_one_sample(oracle, checker, c.osc, True, pw, nw, prm, tmax, 2))
    solid = GpuScene(gpu.dev, dataclasses.replace(c.scene, alpha=None))
    try:
        opaque = gpu.rtao(solid.h, pw, nw, prm, 2)
    finally:
        solid.release()
    assert_frame_equal(opaque, expect_one_sample(oracle, checker, c.osc, False, pw, nw, prm, tmax, 2))
    assert (bits(opaque[1]) != bits(got[1])).sum() >= 20 and (opaque[0] != got[0]).any()


def test_small_max_t_hit(oracle, checker, gpu):
    """maxTHit a tenth of the scene's extent: the checker's frame has at least 5 % hits and 5 % misses, and the GPU's
    is the same frame."""
    c = gpu.cases["opaque"]
    extent = float((c.scene.positions.max(0) - c.scene.positions.min(0)).max())
    _, nw, pw = gpu.gbuffer_world("opaque", False)
    prm = params(gpu, max_t_hit=0.1 * extent)
    tmax = gpu.t_max(prm)
    want = expect_one_sample(oracle, checker, c.osc, c.has_alpha, pw, nw, prm, tmax, 0)
    t = want[2][..., 0, 3]
    print("small maxTHit", tmax, "hits", int((t > 0).sum()), "of", t.size)
    assert (t > 0).mean() >= 0.05 and (t == 0).mean() >= 0.05 and (pw[..., 3] == 1).all()
    assert (t[t > 0] <= tmax).all()
    assert_frame_equal(gpu.rtao(gpu.scenes["opaque"].h, pw, nw, prm, 0), want)


def test_normal_scale_zero(oracle, checker, gpu):
    """normalScale = 0 puts the origins on their surfaces: TMin = 0.001 alone keeps the rays off them.  The checker
    with TMin = 0 gives another frame, so a walk without TMin would show."""
    c = gpu.cases["opaque"]
    _, nw, pw = gpu.gbuffer_world("opaque", True)
    prm = params(gpu, normal_scale=0.0)
    tmax = gpu.t_max(prm)
    want = expect_one_sample(oracle, checker, c.osc, c.has_alpha, pw, nw, prm, tmax, 0)
    orig = RT.origins(checker, pw, nw, 0.0)
    np.testing.assert_array_equal(bits(orig[..., :3])[pw[..., 3] != 0], bits(pw[..., :3])[pw[..., 3] != 0])
    no_tmin = RT.trace(oracle, checker, c.osc, c.has_alpha, orig, want[2][..., 0, :], tmax, tmin=0.0)
    assert (bits(no_tmin[..., 0]) != bits(want[2][..., 0, 3])).mean() >= 0.05
    assert_frame_equal(gpu.rtao(gpu.scenes["opaque"].h, pw, nw, prm, 0), want)


def scalar_bits(v):
    return int(np.float32(v).view(np.uint32))


def shear_ties(d):
    """Rays whose two largest |direction components| are exactly equal.  The watertight triangle test (the
    reference's, restated bit for bit by librsd and by the oracle) picks its shear axis with strict comparisons, so
    such a tie falls back to x however small d.x is; its t then carries rounding errors of about 2^-24 / |d.x| times
    the triangle's size, which can exceed the 1e-5 relative margin of the BVH walk's box test.  For these rays
    "the smallest computed t over all triangles" and "the closest hit of a BVH walk" need not be the same triangle."""
    a = np.sort(np.abs(d[..., :3]), -1)
    return a[..., 2] == a[..., 1]


@pytest.mark.parametrize("name", ["layers_tight", "coincident"])
def test_adversarial_scenes(oracle, checker, gpu, name):
    """Rays from a plane behind the quads of tests/scenes_adversarial.py, straight and slanted through them: 40
    layers 3 float ulps apart (the closest of nearly equal hits) and 10 coincident triangles (exact ties in t).
    Every ray is the checker's bit for bit, except shear-tie rays (shear_ties: with the normal (0, 0, 1) a table
    entry with s.y == s.z gives |d.y| == |d.z|): there the GPU's t must be the computed t of a triangle that the
    brute force lists for that ray, not below the checker's minimum.  Measured on layers_tight, frame 0, pixel
    (60, 39): d = (0.0314, 0.70676, 0.70676), shear axis x, 1 / d.x = 31.8; the walk returns 0.12730980, the t of
    the layers nearest to the origin, the brute force 0.12730913 (45 ulps less) from the 2 x 2 triangle of layer 16,
    which lies 23 layers farther and whose box the walk rightly drops."""
    from rsd.frame import GpuScene
    sc = ADV.make(name)
    osc = oracle.Scene(sc.positions, sc.indices, sc.flags)
    # just behind the farthest layer / between the repeated quad's plane (z = -3) and the stack's next one (-3.125)
    z0 = -2.1 if name == "layers_tight" else -3.0625
    ys, xs = np.mgrid[0:ADV.H, 0:ADV.W]
    pw = np.stack([(xs - 32) / 64.0, (ys - 24) / 64.0, np.full(xs.shape, z0), np.ones(xs.shape)], -1).astype(np.float32)
    nw = np.zeros_like(pw)
    nw[..., 2] = 1.0
    prm = params(gpu, max_t_hit=1.0)
    tmax = gpu.t_max(prm)
    gs = GpuScene(gpu.dev, sc)
    try:
        got = [gpu.rtao(gs.h, pw, nw, prm, f) for f in (0, 1)]
    finally:
        gs.release()
    for f in (0, 1):
        want = expect_one_sample(oracle, checker, osc, False, pw, nw, prm, tmax, f)
        np.testing.assert_array_equal(bits(got[f][2][..., :3]), bits(want[2][..., :3]))  # the rays themselves
        tie = shear_ties(want[2][..., 0, :])
        assert tie.mean() < 0.02  # decided by the directions alone
        for g, w, what in zip(got[f], want, ("ambient", "ray_distance", "ray log")):
            np.testing.assert_array_equal(bits(g)[~tie], bits(w)[~tie], err_msg=what)
        orig = RT.origins(checker, pw, nw, prm.normal_scale)
        for y, x in zip(*np.nonzero(tie)):
            tg, tr = got[f][2][y, x, 0, 3], want[2][y, x, 0, 3]
            if scalar_bits(tg) == scalar_bits(tr):
                continue
            listed = set()
            for prim in range(len(sc.indices)):
                hit, t = oracle.intersect(orig[y, x, :3], want[2][y, x, 0, :3], *sc.positions[sc.indices[prim]])[:2]
                if hit and RT.TMIN <= np.float32(t) <= tmax:
                    listed.add(scalar_bits(t))
            print(f"{name} frame {f} pixel ({x}, {y}): shear-tie ray, t {tg!r} against the brute force's {tr!r}")
            assert scalar_bits(tg) in listed and tg >= tr
            assert got[f][1][y, x] == tg and got[f][0][y, x] == want[0][y, x]
        t = want[2][..., 0, 3]
        assert (t > 0).mean() > 0.9  # the planes span the whole frame: only rays that leave sideways miss
    t = got[0][2][..., 0, 3]
    dz = got[0][2][..., 0, 2]
    near = (t > 0) & ~shear_ties(got[0][2][..., 0, :])
    if name == "coincident":  # the first plane met is z = -3, 0.0625 away: t = 0.0625 / d.z (up to the rounding of d)
        assert np.allclose(t[near] * dz[near], 0.0625 - 0.01, rtol=1e-4)
    else:  # the nearest of the 40 layers from behind is the last one, within 120 ulps of the first
        zs = np.unique(sc.positions[:, 2])
        assert len(zs) == ADV.LAYER_COUNT
        assert np.allclose(t[near] * dz[near], zs.min() - np.float32(z0) - 0.01, rtol=1e-4)


def test_scene_without_triangles(gpu):
    """Every ray misses: ambient 1 and ray_distance maxAORayTHit everywhere, directions still logged."""
    from rsd.frame import GpuScene
    from rsd.scenes import Scene
    empty = Scene("empty", np.zeros((1, 3), np.float32), np.zeros((0, 3), np.uint32), np.zeros(0, np.uint32),
                  gpu.cases["opaque"].scene.camera)
    _, nw, pw = gpu.gbuffer_world("opaque", True)
    gs = GpuScene(gpu.dev, empty)
    try:
        for spp in (1, 4):
            prm = params(gpu, spp=spp, apply_exponential_falloff=True)
            amb, dist, log = gpu.rtao(gs.h, pw, nw, prm, 0)
            valid = pw[..., 3] != 0
            tmax = gpu.t_max(prm)
            # spp rays that all miss: maxAORayTHit, or (maxAORayTHit + spp maxAORayTHit) / spp with the reference's sum
            want = np.where(valid, RT.ray_distance(np.zeros((H, W, spp), np.float32), tmax), tmax)
            assert (amb == 1).all() and (log[..., 3] == 0).all()
            np.testing.assert_array_equal(bits(dist), bits(want))
            assert np.allclose(np.linalg.norm(log[valid][..., :3], axis=-1), 1.0, atol=1e-6)
    finally:
        gs.release()


def test_graph(oracle, checker, gpu):
    """tests/graphs/rtao.py executed three times: the outputs are the direct call's frames 0, 1 and 2 (the pass's
    counter), ambient as round(255 a) and rayDistance rounded to float16; enabled = False clears ambient to 1."""
    from rsd import graph as rg
    c, torch = gpu.cases["opaque"], gpu.torch
    _, nw, pw = gpu.gbuffer_world("opaque", False)
    prm = params(gpu, max_t_hit=1.0)
    text = SCRIPT.read_text()
    assert "'maxTHit': 1.0, 'applyExponentialFalloff': False, 'spp': 1" in text
    g = rg.load_script(SCRIPT)["RTAO"]
    g.set_scene(gpu.scenes["opaque"].h, c.cam)
    g.compile(W, H)
    seen = []
    for frame in range(3):
        g.execute()
        torch.cuda.synchronize()
        a8 = g.output_tensor("RTAO.ambient").cpu().numpy()
        d16 = g.output_tensor("RTAO.rayDistance").cpu().numpy()
        np.testing.assert_array_equal(bits(g.output_tensor("GBufferRaster.posW").cpu().numpy()), bits(pw))
        amb, dist, _ = gpu.rtao(gpu.scenes["opaque"].h, pw, nw, prm, frame)
        np.testing.assert_array_equal(a8, np.floor(amb.astype(np.float64) * 255.0 + 0.5).astype(np.uint8))
        assert d16.dtype == np.float16
        np.testing.assert_array_equal(d16.view(np.uint16), dist.astype(np.float16).view(np.uint16))
        seen.append(d16)
    assert set(np.unique(a8)) == {18, 255}  # round(255 * 0.07) on a hit, 255 on a miss
    assert (seen[0] != seen[1]).any() and (seen[1] != seen[2]).any() and (seen[0] != seen[2]).any()
    g.close()
    off = rg.load_script(text.replace("'spp': 1", "'spp': 1, 'enabled': False"))["RTAO"]
    off.set_scene(gpu.scenes["opaque"].h, c.cam)
    off.compile(W, H)
    off.execute()
    torch.cuda.synchronize()
    assert (off.output_tensor("RTAO.ambient").cpu().numpy() == 255).all()
    off.close()


def test_renderer_rtao(gpu):
    """Renderer.rtao renders its own world G-buffer and equals the direct calls on it."""
    from rsd.frame import FrameConfig, Renderer
    c = gpu.cases["opaque"]
    r = Renderer(c.scene, FrameConfig(visible_w=W, visible_h=H, guard_band=0), gpu_scene=gpu.scenes["opaque"],
                 dev=gpu.dev)
    _, nw, pw = gpu.gbuffer_world("opaque", False, cull=r.cfg.cull_mode)
    for spp, frame, kw in ((1, 0, dict(max_t_hit=MAX_T, apply_exponential_falloff=False)), (4, 5, dict(max_t_hit=MAX_T))):
        amb, dist = r.rtao(spp=spp, frame_index=frame, **kw)
        gpu.torch.cuda.synchronize()
        want = gpu.rtao(gpu.scenes["opaque"].h, pw, nw, gpu.abi.RTAOParams(spp=spp, **kw), frame)
        np.testing.assert_array_equal(bits(amb.cpu().numpy()), bits(want[0]))
        np.testing.assert_array_equal(bits(dist.cpu().numpy()), bits(want[1]))
    assert (want[0] < 1).any()
