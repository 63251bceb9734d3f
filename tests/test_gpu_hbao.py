"""GPU: rsd_hbao, Renderer.hbao, the HBAO graph pass and rsd_cross_bilateral_blur_src against the scalar CPU
checker (tests/native/hbao_ref.c, whose known answers and input conditions tests/test_hbao.py asserts).  Every
comparison is on the RG8Unorm / R8Unorm bytes, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import hbao_checker as HB
from conftest import ROOT
from helpers import small_frame_config

pytestmark = pytest.mark.gpu
F = np.float32
SCRIPT = ROOT / "tests" / "graphs" / "hbao.py"
MODES = {"SingleDepth": HB.SINGLE, "DualDepth": HB.DUAL}


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return HB.build(tmp_path_factory.mktemp("hbao_ref"))


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def inputs(torch):
    """The synthetic inputs, built once, uploaded once and shared (read-only) by every parameter point."""
    out = {}
    for size in HB.SIZES:
        s = HB.synthetic(*size)
        s["dev"] = {k: torch.from_numpy(np.array(s[k])).cuda() for k in ("layers", "layers2", "normal_w")}
        out[size] = s
    return out


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("exponent", HB.EXPONENTS)
@pytest.mark.parametrize("radius_index", [0, 1, 2], ids=["r_all", "r_some", "r_few"])
@pytest.mark.parametrize("guard", HB.GUARDS)
@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES))
@pytest.mark.parametrize("size", HB.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_parity(torch, checker, inputs, size, mode, guard, radius_index, exponent):
    """rsd_hbao equals the checker bit for bit on the RG8 bytes; the sentinel bytes of the output remain exactly
    on the scissored texels; the inputs are untouched."""
    from rsd import abi
    s, (W, H) = inputs[size], size
    d = s["dev"]
    radius = HB.radii(H)[radius_index]
    qh, qw = s["layers"].shape[1:]
    out = torch.full((16, qh, qw, 2), HB.SENTINEL, dtype=torch.uint8, device="cuda")
    prm = abi.HBAOParams(radius=radius, power_exponent=exponent, depth_mode=MODES[mode], guard_band=guard)
    abi.check(abi.lib().rsd_hbao(_p(d["layers"]), _p(d["layers2"]) if MODES[mode] == HB.DUAL else None,
                                 _p(d["normal_w"]), W, H, C.byref(s["cam"]), C.byref(prm), _p(out), _stream(torch)),
              "rsd_hbao")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want, flags = HB.hbao(checker, s["layers"], s["layers2"], s["normal_w"], s["cam"], radius=radius,
                          exponent=exponent, depth_mode=MODES[mode], guard_band=guard)
    diff = (got != want).any(-1)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5], got[diff][:5], want[diff][:5], flags[diff][:5])
    scissored = (flags & HB.SCISSORED) != 0
    assert scissored.sum() == HB.scissored_texels(W, H, guard)
    assert (got[scissored] == HB.SENTINEL).all()
    # ... and nowhere else: no answer inside the scissor is the sentinel pair (tests/test_hbao.py asserts that on
    # the checker for every parameter point), so a texel left unwritten would have differed above
    assert not (got[~scissored] == HB.SENTINEL).all(-1).any()
    for k in ("layers", "layers2", "normal_w"):
        assert np.array_equal(d[k].cpu().numpy().view(np.uint32), np.asarray(s[k]).view(np.uint32)), k


def test_taps_between_two_texels_round_to_even(torch, checker):
    """HB.tie_case (taps at exactly 1.5 and 2.5 quarter texels, a caller's Rand table): rsd_hbao equals the checker,
    which tests/test_hbao.py shows to send 2.5 to texel 2."""
    from rsd import abi
    t = HB.tie_case()
    W, H = 64, 48
    layers, normals = torch.from_numpy(t["layers"]).cuda(), torch.from_numpy(np.array(t["normal_w"])).cuda()
    out = torch.full((16, H // 4, W // 4, 2), HB.SENTINEL, dtype=torch.uint8, device="cuda")
    prm = abi.HBAOParams(radius=t["radius"], rand=t["rand"])
    abi.check(abi.lib().rsd_hbao(_p(layers), None, _p(normals), W, H, C.byref(t["cam"]), C.byref(prm), _p(out),
                                 _stream(torch)), "rsd_hbao")
    torch.cuda.synchronize()
    want, flags = HB.hbao(checker, t["layers"], None, t["normal_w"], t["cam"], radius=t["radius"], rand=t["rand"])
    assert ((flags & HB.TIE) != 0).mean() > 0.95
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("guard", HB.GUARDS)
def test_blur_reads_the_first_channel_of_an_rg8_source(torch, guard):
    """rsd_cross_bilateral_blur_src with 2-byte source texels equals rsd_cross_bilateral_blur on the extracted
    first channel, byte for byte (150 x 90, radius 4), and with 1-byte texels it is that function."""
    from rsd import abi
    W, H = 150, 90
    rng = np.random.default_rng(11 + guard)
    rg = torch.from_numpy(rng.integers(0, 256, (H, W, 2), dtype=np.uint8)).cuda()
    z = torch.from_numpy((3.0 + np.cumsum(rng.normal(0, 0.02, (H, W)), axis=1)).astype(F)).cuda()
    first = rg[..., 0].contiguous()
    L, st = abi.lib(), _stream(torch)
    outs = []
    for call in ("plain", "src1", "src2"):
        ping = torch.full((H, W), HB.SENTINEL, dtype=torch.uint8, device="cuda")
        dst = torch.full((H, W), HB.SENTINEL, dtype=torch.uint8, device="cuda")
        if call == "plain":
            abi.check(L.rsd_cross_bilateral_blur(_p(first), _p(z), W, H, _p(ping), _p(dst), W, H, guard, 4, 1, st), call)
        else:
            src, nbytes = (first, 1) if call == "src1" else (rg, 2)
            abi.check(L.rsd_cross_bilateral_blur_src(_p(src), nbytes, _p(z), W, H, _p(ping), _p(dst), W, H, guard, 4, 1,
                                                     st), call)
        torch.cuda.synchronize()
        outs.append((ping.cpu().numpy(), dst.cpu().numpy()))
    for ping, dst in outs[1:]:
        assert np.array_equal(ping, outs[0][0]) and np.array_equal(dst, outs[0][1])
    dst = outs[0][1]
    inner = dst[guard:H - guard, guard:W - guard]
    assert len(np.unique(inner)) > 50
    if guard:
        border = np.ones((H, W), bool)
        border[guard:H - guard, guard:W - guard] = False
        assert (dst[border] == HB.SENTINEL).all()
    # the second channel is not read: another one gives the same bytes
    rg2 = rg.clone()
    rg2[..., 1] = 255 - rg2[..., 1]
    ping, dst2 = torch.zeros_like(first), torch.full((H, W), HB.SENTINEL, dtype=torch.uint8, device="cuda")
    abi.check(L.rsd_cross_bilateral_blur_src(_p(rg2), 2, _p(z), W, H, _p(ping), _p(dst2), W, H, guard, 4, 1, st), "src2")
    torch.cuda.synchronize()
    assert np.array_equal(dst2.cpu().numpy(), dst)


@pytest.fixture(scope="module")
def arcade(torch):
    from rsd.frame import Device, GpuScene
    from rsd.scenes import make_scene
    scene = make_scene("arcade_tiny")
    dev = Device(0)
    gs = GpuScene(dev, scene)
    yield dict(scene=scene, dev=dev, gs=gs)
    gs.release()
    dev.close()


def test_renderer_hbao(torch, checker, arcade):
    """Renderer.hbao on arcade_tiny at small_frame_config(): the full-size (bright, dark) map equals the checker
    fed the renderer's own linear depth and face normals, in SingleDepth and, with the peeled second layer, in
    DualDepth; the scene darkens some pixels and the guard band keeps the cleared value."""
    from rsd import abi
    from rsd.frame import Renderer
    cfg = small_frame_config()
    cfg.primary = abi.DEPTH_DUAL
    W, H, g = cfg.fb_w, cfg.fb_h, cfg.guard_band
    r = Renderer(arcade["scene"], cfg, gpu_scene=arcade["gs"], dev=arcade["dev"])
    r.gbuffer()
    r.depth_peel(0.5)
    results = {}
    for mode in (abi.DEPTH_SINGLE, abi.DEPTH_DUAL):
        got = r.hbao(depth_mode=mode, radius=1.0)
        torch.cuda.synchronize()
        assert tuple(got.shape) == (H, W, 2) and got.dtype == torch.uint8
        z, z2, n = r.depth.cpu().numpy(), r.depth2.cpu().numpy(), r.face_normal_w.cpu().numpy()
        want_layers, flags = HB.hbao(checker, HB.deinterleave(z), HB.deinterleave(z2), n, r.cam, radius=1.0,
                                     depth_mode=mode, guard_band=g, fill=255)
        want = HB.interleave(want_layers, W, H)
        got = got.cpu().numpy()
        assert np.array_equal(got, want), int((got != want).sum())
        results[mode] = got
    one, two = results[abi.DEPTH_SINGLE], results[abi.DEPTH_DUAL]
    assert (one < 255).mean() > 0.02 and (one[g:H - g, g:W - g] < 255).any()
    assert (one[:g] == 255).all() and (one[:, :g] == 255).all()
    assert (two <= one).all() and (two < one).any()
    with pytest.raises(ValueError):
        r.hbao(depth_mode=abi.DEPTH_DUAL, depth2=r.depth2[:10])
    with pytest.raises(abi.RsdError):
        r.hbao(depth_mode=abi.DEPTH_STOCHASTIC)


@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES))
def test_graph(torch, checker, arcade, mode):
    """tests/graphs/hbao.py executed: HBAO.ambientMap equals the checker on the graph's own layers and normals
    (outside the guard-band scissor it keeps the cleared zeros), the final image's red channel is the blur of the
    interleaved bright channel, and a second execute gives the same bytes."""
    from rsd import abi
    from rsd import graph as rg
    from rsd.frame import look_at
    scene, gs = arcade["scene"], arcade["gs"]
    cfg = small_frame_config()
    W, H = cfg.fb_w, cfg.fb_h
    text = SCRIPT.read_text()
    assert "'depthMode': 'DualDepth'" in text
    g = rg.load_script(text.replace("'depthMode': 'DualDepth'", f"'depthMode': '{mode}'"))["HBAOGraph"]
    cam = look_at(scene.camera["pos"], scene.camera["target"], scene.camera["up"], cfg)
    g.set_scene(gs.h, cam)
    g.compile(W, H)
    g.execute()
    torch.cuda.synchronize()
    guard = g.dict_int("guardBand")
    assert guard == 16
    np_ = lambda name: g.output_tensor(name).cpu().numpy()  # noqa: E731
    layers, layers2 = np_("DeinterleaveDepth.texOut"), np_("DeinterleaveDepth2.texOut")
    normals = np_("GBufferRaster.faceNormalW").reshape(H, W, 4)
    ambient = np_("HBAO.ambientMap")
    want, flags = HB.hbao(checker, layers, layers2, normals, cam, radius=1.0, bias=0.1, exponent=2.0,
                          depth_mode=MODES[mode], guard_band=guard, fill=0)
    assert ambient.shape == want.shape
    assert np.array_equal(ambient, want), int((ambient != want).sum())
    assert ((ambient < 255) & (ambient > 0)).mean() > 0.02
    if MODES[mode] == HB.DUAL:
        single, _ = HB.hbao(checker, layers, None, normals, cam, guard_band=guard, fill=0)
        assert (HB.recompute_count(flags) > 0).mean() > 0.02 and (single != ambient).any()
    # the blur reads the bright channel of the interleaved map; Ambient shows it as grey
    inter = np_("InterleaveAO.texOut").reshape(H, W, 2)
    assert np.array_equal(inter, HB.interleave(ambient, W, H))
    z = g.output_tensor("LinearizeDepth.linearDepth").reshape(H, W).contiguous()
    bright = torch.from_numpy(np.ascontiguousarray(inter[..., 0])).cuda()
    ping, blurred = torch.zeros_like(bright), torch.zeros_like(bright)
    abi.check(abi.lib().rsd_cross_bilateral_blur(_p(bright), _p(z), W, H, _p(ping), _p(blurred), W, H, guard, 4, 1,
                                                 _stream(torch)), "rsd_cross_bilateral_blur")
    torch.cuda.synchronize()
    blurred = blurred.cpu().numpy()
    assert np.array_equal(np_("BlurAO.colorOut").reshape(H, W), blurred)
    final = np_("Ambient.out").reshape(H, W, 4)
    assert np.array_equal(np.rint(final[..., 0] * 255.0).astype(np.uint8), blurred)
    assert np.array_equal(final[..., 0], final[..., 1]) and np.array_equal(final[..., 0], final[..., 2])
    assert len(np.unique(blurred)) > 20
    # a second execute gives the same bytes
    g.execute()
    torch.cuda.synchronize()
    assert np.array_equal(np_("HBAO.ambientMap"), ambient)
    assert np.array_equal(np_("Ambient.out").reshape(H, W, 4), final)
    g.close()
