"""GPU: the AOGuidedBlur graph pass and Renderer.ao_guided_blur / ao_variance_fix on the arcade_tiny fixture scene
(tests/graphs/svao_dual_resolve.py), against the scalar CPU checker fed the graph's own marked outputs.  Bit for bit
on the R8Unorm bytes."""
import numpy as np
import pytest

import ao_resolve_checker as AR
from conftest import ROOT
from helpers import small_frame_config

pytestmark = pytest.mark.gpu
SCRIPT = ROOT / "tests" / "graphs" / "svao_dual_resolve.py"


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return AR.build(tmp_path_factory.mktemp("ao_resolve_ref"))


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def arcade(torch):
    from rsd.frame import Device, GpuScene, look_at
    from rsd.scenes import make_scene
    scene = make_scene("arcade_tiny")
    dev = Device(0)
    gs = GpuScene(dev, scene)
    cfg = small_frame_config()
    cam = look_at(scene.camera["pos"], scene.camera["target"], scene.camera["up"], cfg)
    yield dict(scene=scene, dev=dev, gs=gs, cfg=cfg, cam=cam)
    gs.release()
    dev.close()


def _run(torch, arcade, name, text=None):
    from rsd import graph as rg
    cfg = arcade["cfg"]
    g = rg.load_script(SCRIPT if text is None else text)[name]
    g.set_scene(arcade["gs"].h, arcade["cam"])
    g.compile(cfg.fb_w, cfg.fb_h)
    g.execute()
    torch.cuda.synchronize()
    return g


def test_svao_dual_ao_graph(torch, checker, arcade):
    """SVAO (dualAO) -> DeinterleaveTexture x 2 -> AOGuidedBlur -> InterleaveTexture -> CrossBilateralBlur ->
    ImageEquation: AOGuidedBlur.color equals the checker on the numpy-deinterleaved SVAO.ao and linear depth (the
    texels outside the scissor keep the cleared zeros), the blur's source is its interleaved image, and a second
    execute gives the same bytes."""
    cfg = arcade["cfg"]
    W, H = cfg.fb_w, cfg.fb_h
    g = _run(torch, arcade, "SVAODualResolve")
    guard = g.dict_int("guardBand")
    assert guard == 16
    np_ = lambda name: g.output_tensor(name).cpu().numpy()  # noqa: E731
    ao2 = np_("SVAO.ao").reshape(H, W, 2)
    z = np_("LinearizeDepth.linearDepth").reshape(H, W)
    assert (ao2[..., 0] != ao2[..., 1]).any()  # the pair differs somewhere: there is something to resolve
    color = np_("AOGuidedBlur.color")
    want, _, n = AR.guided_blur(checker, AR.deinterleave(ao2), AR.deinterleave(z), W, H, guard, 2, True, fill=0)
    assert color.shape == want.shape == (16, H // 4, W // 4)
    assert np.array_equal(color, want), (int((color != want).sum()), np.argwhere(color != want)[:5])
    assert n["tap_zero"] > 0 and n["tap_half"] > 0 and n["ldev_kept"] > 0 and n["ldev_raised"] > 0
    m = AR.inside(W, H, 16, guard)
    assert len(np.unique(color[m])) > 20
    final = np_("Ambient.out").reshape(H, W, 4)
    assert np.array_equal(final[..., 0], final[..., 1]) and len(np.unique(final[..., 0])) > 20
    g.execute()
    torch.cuda.synchronize()
    assert np.array_equal(np_("AOGuidedBlur.color"), color) and np.array_equal(np_("Ambient.out").reshape(H, W, 4), final)
    g.close()


def test_disabled_pass_copies_the_first_channel(torch, arcade):
    """'enabled': False (what scripts/SVAO_depth.py sets): color is byte 0 of every ao2 texel, the reference's blit
    into the R8Unorm target, without a scissor."""
    cfg = arcade["cfg"]
    W, H = cfg.fb_w, cfg.fb_h
    text = SCRIPT.read_text()
    assert text.count("'clampResults': True, 'enabled': True}") == 1
    g = _run(torch, arcade, "SVAODualResolve",
             text.replace("'clampResults': True, 'enabled': True}", "'clampResults': True, 'enabled': False}"))
    ao2 = g.output_tensor("SVAO.ao").cpu().numpy().reshape(H, W, 2)
    color = g.output_tensor("AOGuidedBlur.color").cpu().numpy()
    assert np.array_equal(color, AR.deinterleave(ao2[..., 0]))
    assert len(np.unique(color)) > 20
    g.close()


def test_hbao_layers_feed_the_pass_directly(torch, checker, arcade):
    """HBAO.ambientMap, 16 RG8Unorm layers, straight into AOGuidedBlur (radius 4, no local deviation)."""
    cfg = arcade["cfg"]
    W, H = cfg.fb_w, cfg.fb_h
    g = _run(torch, arcade, "HBAOResolve")
    guard = g.dict_int("guardBand")
    np_ = lambda name: g.output_tensor(name).cpu().numpy()  # noqa: E731
    ambient = np_("HBAO.ambientMap").reshape(16, H // 4, W // 4, 2)
    layers = np_("DeinterleaveDepth.texOut").reshape(16, H // 4, W // 4)
    color = np_("AOGuidedBlur.color")
    want, _, n = AR.guided_blur(checker, ambient, layers, W, H, guard, 4, False, fill=0)
    assert np.array_equal(color, want), (int((color != want).sum()), np.argwhere(color != want)[:5])
    assert n["adev_kept"] > 0 and len(np.unique(color)) > 20
    assert np.array_equal(np_("InterleaveAO.texOut").reshape(H, W), AR.interleave(color, W, H))
    g.close()


def test_renderer_methods(torch, checker, arcade):
    """Renderer.ao_guided_blur on the (bright, dark) map of a dual_ao frame and Renderer.ao_variance_fix on its two
    channels: both equal the checker fed the renderer's own AO map and linear depth; bad shapes are refused."""
    from rsd.frame import Renderer
    cfg = small_frame_config()
    cfg.dual_ao = True
    W, H, g = cfg.fb_w, cfg.fb_h, cfg.guard_band
    r = Renderer(arcade["scene"], cfg, gpu_scene=arcade["gs"], dev=arcade["dev"])
    r.gbuffer()
    r.frame()
    torch.cuda.synchronize()
    ao2, z = r.ao.cpu().numpy(), r.depth.cpu().numpy()
    assert ao2.shape == (H, W, 2)
    for radius, ldev in ((4, True), (2, False)):
        got = r.ao_guided_blur(kernel_radius=radius, local_deviation=ldev)
        torch.cuda.synchronize()
        want, _, _ = AR.guided_blur(checker, AR.deinterleave(ao2), AR.deinterleave(z), W, H, g, radius, ldev, fill=0)
        assert tuple(got.shape) == (H, W) and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), AR.interleave(want, W, H))
    one = r.ao_guided_blur(ao2=r.ao[..., 0].contiguous(), kernel_radius=2).cpu().numpy()
    want, _, _ = AR.guided_blur(checker, AR.deinterleave(ao2[..., 0]), AR.deinterleave(z), W, H, g, 2, True, fill=0)
    assert np.array_equal(one, AR.interleave(want, W, H))
    fix = r.ao_variance_fix(r.ao[..., 0].contiguous(), r.ao[..., 1].contiguous()).cpu().numpy()
    want, _ = AR.variance_fix(checker, AR.deinterleave(ao2[..., 0]), AR.deinterleave(ao2[..., 1]), AR.deinterleave(z),
                              W, H, g, fill=0)
    assert np.array_equal(fix, AR.interleave(want, W, H)) and len(np.unique(fix)) > 20
    with pytest.raises(ValueError):
        r.ao_guided_blur(ao2=r.ao[:10])
    with pytest.raises(ValueError):
        r.ao_variance_fix(r.ao, r.ao)
