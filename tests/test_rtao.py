"""CPU checks of the RTAO feature (rsd_rtao, rsd_gbuffer_world, the RTAO graph pass): the generators' known
answers, the sample table against the checker's and against float64, the argument refusals of the C entries
(no GPU needed), the pass's registration and reflection, and the untouched older G-buffer entry points."""
import ctypes as C
import re
import shutil
import subprocess

import numpy as np
import pytest

import rtao_checker as RT
from conftest import ROOT

rsdgraph = pytest.importorskip("rsd.graph")
from rsd import abi  # noqa: E402

SCRIPT = ROOT / "tests" / "graphs" / "rtao.py"
needs_gcc = pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")


@pytest.fixture(scope="session")
def checker(oracle, tmp_path_factory):
    return RT.build(oracle, tmp_path_factory.mktemp("rtao_ref"))


def lib_table():
    t = np.zeros(abi.RTAO_SAMPLE_COUNT, np.uint32)
    abi.check(abi.lib().rsd_rtao_sample_table(t.ctypes.data), "rsd_rtao_sample_table")
    return t


@needs_gcc
def test_mt19937_known_answer(checker):
    """std::mt19937(89): the checker's generator and numpy's give the first raw draws of the reference's."""
    want = [2146170771, 1665720606, 1099241604]
    assert RT.mt_raw(checker, 89, 3).tolist() == want
    g = np.random.MT19937()
    g._legacy_seeding(89)
    assert g.random_raw(3).tolist() == want
    # the 10000th draw of mt19937(5489), the value the C++ standard requires
    assert RT.mt_raw(checker, 5489, 10000)[-1] == 4123659995


@needs_gcc
def test_sample_table_matches_the_checker(checker):
    assert abi.RTAO_SAMPLE_COUNT == RT.SAMPLES == 5312
    np.testing.assert_array_equal(lib_table(), RT.table(checker))


def test_sample_table_matches_float64():
    """Every component equals the rounding of its float64 value, those within 1e-4 of a rounding tie left out
    (6 of 15936 on this table; at most 8 may be left out); w is 0; the samples are a cosine-weighted hemisphere."""
    t = lib_table()
    got = np.stack([(t >> (8 * k)) & 0xff for k in range(3)], -1).astype(np.uint8).view(np.int8).astype(np.int64)
    v = RT.table_float64()
    near_tie = np.abs(np.abs(v - np.floor(v)) - 0.5) < 1e-4
    assert near_tie.sum() <= 8, int(near_tie.sum())
    want = np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5)).astype(np.int64)  # round half away from zero
    np.testing.assert_array_equal(got[~near_tie], want[~near_tie])
    assert (np.abs(got - want) <= 1).all()
    assert ((t >> 24) == 0).all()
    assert (got[:, 2] >= 0).all() and abs((got[:, 2] / 127.0).mean() - 2.0 / 3.0) < 0.01  # E[cos] = 2/3
    assert abs(got[:, 0].mean()) < 2.0 and abs(got[:, 1].mean()) < 2.0


@needs_gcc
def test_hash_and_jenkins_known_answers(checker):
    """Ray.rt.slang:61-77 evaluated by hand in numpy uint32 arithmetic, against the checker's C."""
    def jenkins_scalar(a):
        m = 0xffffffff
        a = (a - (a << 6)) & m
        a ^= a >> 17
        a = (a - (a << 9)) & m
        a ^= (a << 4) & m
        a = (a - (a << 3)) & m
        a ^= (a << 10) & m
        a ^= a >> 15
        return a

    for a in (0, 1, 7, 89, 0x12345678, 0xffffffff):
        assert int(RT.jenkins(np.uint32(a))) == jenkins_scalar(a) == checker.rtao_jenkins_ref(a)
    assert jenkins_scalar(0) == 0 and jenkins_scalar(1) != 1
    for x, y, f in ((0, 0, 0), (74, 44, 7), (1919, 1079, 123456), (3, 5, 0xffffffff)):
        want = jenkins_scalar((x * 449 + y * 2857 + jenkins_scalar(f)) & 0xffffffff)
        assert int(RT.pixel_hash(x, y, f)) == want == checker.rtao_hash_ref(x, y, f)
    # the frame index and both coordinates reach the table index
    idx = RT.pixel_hash(*np.meshgrid(np.arange(75), np.arange(45)), 0) % RT.SAMPLES
    assert len(np.unique(idx)) > 0.25 * idx.size
    assert (RT.pixel_hash(*np.meshgrid(np.arange(75), np.arange(45)), 1) % RT.SAMPLES != idx).mean() > 0.99


def test_xoshiro_known_answers():
    """SplitMix64 and xoshiro128** against their authors' published C, evaluated here with Python integers;
    interleave_32bit against bit-by-bit interleaving."""
    M64, M32 = (1 << 64) - 1, (1 << 32) - 1

    def splitmix(state):
        state = (state + 0x9E3779B97F4A7C15) & M64
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return state, z ^ (z >> 31)

    # SplitMix64 from state 0: the first output of the public-domain reference implementation
    assert splitmix(0)[1] == 0xE220A8397B1DCDAF

    def rotl(x, k):
        return ((x << k) | (x >> (32 - k))) & M32

    def generator(x, y, frame, n):
        morton = 0
        for b in range(16):
            morton |= ((x >> b) & 1) << (2 * b) | ((y >> b) & 1) << (2 * b + 1)
        st, a = splitmix((frame << 32) | morton)
        st, b = splitmix(st)
        s = [a & M32, a >> 32, b & M32, b >> 32]
        out = []
        for _ in range(n):
            out.append((rotl((s[0] * 5) & M32, 7) * 9) & M32)
            t = (s[1] << 9) & M32
            s[2] ^= s[0]
            s[3] ^= s[1]
            s[1] ^= s[2]
            s[0] ^= s[3]
            s[2] ^= t
            s[3] = rotl(s[3], 11)
        return out

    # xoshiro128** from the state {1, 2, 3, 4}: rotl(1 * 5, 7) * 9 = 5760 first
    assert (rotl(1 * 5, 7) * 9) & M32 == 5760
    for x, y, f in ((0, 0, 0), (74, 44, 7), (5, 3, 1), (0xffff, 0xabcd, 0xffffffff)):
        assert RT.uniform_generator(x, y, f, 8).tolist() == generator(x, y, f, 8)
    xs, ys = np.meshgrid(np.arange(75), np.arange(45))
    g = RT.uniform_generator(xs, ys, 7, 4)
    assert g.shape == (4, 45, 75) and g[:, 44, 74].tolist() == generator(74, 44, 7, 4)


def test_rtao_arguments_are_checked():
    """rsd_rtao, rsd_rtao_ray_t_max, rsd_gbuffer_world, rsd_rtao_pack and rsd_rtao_sample_table refuse bad
    arguments on the host (status 1 and a message naming the function), before any GPU work."""
    L = abi.lib()
    d = C.c_void_p(16)  # never dereferenced: the checks come first
    good = abi.RTAOParams()
    ok = dict(scene=d, prm=good, w=8, h=8, pos=d, nrm=d, amb=d, dist=d)

    def call(**kw):
        a = {**ok, **kw}
        prm = C.byref(a["prm"]) if a["prm"] is not None else None
        return L.rsd_rtao(a["scene"], prm, a["w"], a["h"], a["pos"], a["nrm"], 0, a["amb"], a["dist"], None, None)

    bad_params = [abi.RTAOParams(spp=0), abi.RTAOParams(max_t_hit=0.0), abi.RTAOParams(max_t_hit=-1.0),
                  abi.RTAOParams(max_t_hit=float("inf")), abi.RTAOParams(max_t_hit=float("nan")),
                  abi.RTAOParams(min_occlusion_cutoff=0.0), abi.RTAOParams(min_occlusion_cutoff=1.0),
                  abi.RTAOParams(min_occlusion_cutoff=1.5), abi.RTAOParams(min_occlusion_cutoff=float("nan")),
                  abi.RTAOParams(exponential_falloff_decay_constant=0.0)]
    for bad in [dict(scene=None), dict(prm=None), dict(pos=None), dict(nrm=None), dict(amb=None), dict(dist=None),
                dict(w=0), dict(h=0)] + [dict(prm=p) for p in bad_params]:
        assert call(**bad) == abi.ERR_INVALID_ARG, bad
        assert b"rsd_rtao" in L.rsd_last_error(), bad
    t = C.c_float()
    for p in bad_params:
        assert L.rsd_rtao_ray_t_max(C.byref(p), C.byref(t)) == abi.ERR_INVALID_ARG
        assert b"rsd_rtao_ray_t_max" in L.rsd_last_error()
    assert L.rsd_rtao_ray_t_max(None, C.byref(t)) == abi.ERR_INVALID_ARG
    assert L.rsd_rtao_ray_t_max(C.byref(good), None) == abi.ERR_INVALID_ARG
    # without the falloff the cutoff and the decay constant are not read
    off = abi.RTAOParams(apply_exponential_falloff=False, min_occlusion_cutoff=7.0, exponential_falloff_decay_constant=0.0,
                         max_t_hit=0.25)
    assert L.rsd_rtao_ray_t_max(C.byref(off), C.byref(t)) == abi.RSD_OK and t.value == 0.25
    # RTAO.cpp:134-141 with the defaults: sqrt(ln(0.4) / -2) * 1, within float32 rounding of the float64 value
    assert L.rsd_rtao_ray_t_max(C.byref(good), C.byref(t)) == abi.RSD_OK
    assert abs(t.value - np.sqrt(np.log(np.float64(np.float32(0.4))) / -2.0)) < 2e-7
    cam = abi.Camera()
    for a in [(None, C.byref(cam), 8, 8, 1, d, d, d), (d, None, 8, 8, 1, d, d, d), (d, C.byref(cam), 0, 8, 1, d, d, d),
              (d, C.byref(cam), 8, 0, 1, d, d, d), (d, C.byref(cam), 8, 8, 3, d, d, d),
              (d, C.byref(cam), 8, 8, 1, None, d, d), (d, C.byref(cam), 8, 8, 1, d, None, d),
              (d, C.byref(cam), 8, 8, 1, d, d, None)]:
        assert L.rsd_gbuffer_world(*a, None) == abi.ERR_INVALID_ARG, a
        assert b"rsd_gbuffer_world" in L.rsd_last_error(), a
    assert L.rsd_rtao_sample_table(None) == abi.ERR_INVALID_ARG
    for a in [(None, None, 4, None, None), (d, None, 4, None, None), (None, d, 4, d, None), (d, None, 0, d, None)]:
        assert L.rsd_rtao_pack(*a, None) == abi.ERR_INVALID_ARG, a
        assert b"rsd_rtao_pack" in L.rsd_last_error(), a


def test_rtao_params_layout(tmp_path):
    src = '#include <stdio.h>\n#include "rsd.h"\nint main(void){printf("%zu %d\\n", sizeof(rsd_rtao_params), ' \
          '(int)RSD_RTAO_SAMPLE_COUNT);return 0;}\n'
    (tmp_path / "s.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [C.sizeof(abi.RTAOParams), abi.RTAO_SAMPLE_COUNT]
    p = abi.RTAOParams()  # the defaults of RTAO.h / RTAOData.slang
    assert (p.max_t_hit, p.apply_exponential_falloff, p.exponential_falloff_decay_constant, p.spp) == (1.0, 1, 2.0, 1)
    assert (np.float32(p.min_occlusion_cutoff), np.float32(p.minimum_ambient_illumination), np.float32(p.normal_scale)) \
        == (np.float32(0.4), np.float32(0.07), np.float32(0.01))


def test_rtao_is_a_builtin_pass_and_its_script_plans():
    assert "RTAO" in rsdgraph.plugin_types()
    g = rsdgraph.load_script(SCRIPT)["RTAO"]
    g.plan(RT.W, RT.H)
    order = g.execution_order()
    assert order == ["GBufferRaster", "RTAO"]
    res = g.resources()
    assert res["RTAO.ambient"] == (RT.W, RT.H, 1, "R8Unorm")  # RTAO.cpp:69-70
    assert res["RTAO.rayDistance"] == (RT.W, RT.H, 1, "R16Float")
    assert res["GBufferRaster.posW"] == (RT.W, RT.H, 1, "RGBA32Float")
    assert res["GBufferRaster.faceNormalW"] == (RT.W, RT.H, 1, "RGBA32Float")
    assert "GBufferRaster.mvec" not in res


def test_posw_is_allocated_only_when_read():
    g = rsdgraph.RenderGraph("g")
    g.create_pass("GBufferRaster", "GBufferRaster", {})
    g.mark_output("GBufferRaster.depth")
    g.plan(64, 32)
    assert "GBufferRaster.posW" not in g.resources() and "GBufferRaster.depth" in g.resources()


def test_rtao_pass_properties():
    g = rsdgraph.RenderGraph("g")
    g.create_pass("A", "RTAO", {})  # the reference's pass takes none
    g.create_pass("B", "RTAO", {"enabled": False, "maxTHit": 0.5, "normalScale": 0.0, "applyExponentialFalloff": True,
                                "minOcclusionCutoff": 0.2, "exponentialFalloffDecayConstant": 4.0,
                                "minimumAmbientIllumination": 0.1, "spp": 4, "someFutureKey": 1})
    for bad, msg in (({"spp": 0}, "spp"), ({"maxTHit": 0.0}, "max_t_hit"), ({"minOcclusionCutoff": 1.0}, "cutoff"),
                     ({"exponentialFalloffDecayConstant": 0.0}, "decay")):
        with pytest.raises(abi.RsdError, match=msg):
            g.create_pass("C", "RTAO", bad)
    # an unconnected required input is reported when the graph is planned
    h = rsdgraph.RenderGraph("h")
    h.create_pass("GBufferRaster", "GBufferRaster", {})
    h.create_pass("RTAO", "RTAO", {})
    h.add_edge("GBufferRaster.posW", "RTAO.wPos")
    h.mark_output("RTAO.ambient")
    with pytest.raises(abi.RsdError, match="faceNormal"):
        h.plan(64, 32)


def test_older_gbuffer_entry_points_are_unchanged():
    """rsd_gbuffer and rsd_gbuffer_raster keep their declarations and still export; rsd_gbuffer_world and the
    RTAO entries are additions under the same ABI version."""
    text = re.sub(r"\s+", " ", (ROOT / "include" / "rsd.h").read_text())
    assert ("rsd_status rsd_gbuffer(rsd_scene* scene, const rsd_camera* cam, uint32_t width, uint32_t height, "
            "uint32_t cull_mode, float* d_linear_z, uint16_t* d_normals, rsd_stream stream);") in text
    assert ("rsd_status rsd_gbuffer_raster(rsd_scene* scene, const rsd_camera* cam, uint32_t width, uint32_t height, "
            "uint32_t cull_mode, float* d_depth, float* d_normal_w, rsd_stream stream);") in text
    assert "#define RSD_ABI_VERSION 8" in text
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (rsd_\w+)", out))
    assert {"rsd_gbuffer", "rsd_gbuffer_raster", "rsd_gbuffer_world", "rsd_rtao", "rsd_rtao_sample_table",
            "rsd_rtao_ray_t_max", "rsd_rtao_pack"} <= exported
    assert abi.lib().rsd_abi_version() == 8
