"""GPU: the ConvolutionalNet graph pass and Renderer.convnet on the arcade_tiny fixture scene
(tests/graphs/svao_convnet.py, a 70 x 38 frame with guard band 8), against the scalar CPU checker fed the graph's own
deinterleaved resources.  Exact numerics: the floats are equal."""
import numpy as np
import pytest

import convnet_checker as CN
from conftest import ROOT
from helpers import small_frame_config

pytestmark = pytest.mark.gpu
SCRIPT = ROOT / "tests" / "graphs" / "svao_convnet.py"


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return CN.build(tmp_path_factory.mktemp("convnet_ref"))


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
    cfg = small_frame_config(visible=(54, 22), guard=8)
    cam = look_at(scene.camera["pos"], scene.camera["target"], scene.camera["up"], cfg)
    yield dict(scene=scene, dev=dev, gs=gs, cfg=cfg, cam=cam)
    gs.release()
    dev.close()


def test_svao_convnet_graph(torch, checker, arcade, tmp_path, monkeypatch):
    """SVAO (dualAO) -> ExtractBright / ExtractDark / ImageEquation1 / depth / 1000 -> DeinterleaveTexture x 4 ->
    ConvolutionalNet -> InterleaveTexture -> ImageEquation: ConvolutionalNet.out equals the checker on the graph's own
    deinterleaved layers with the "%g"-rounded net A (the texels outside the scissor keep the cleared zeros), the
    interleaved image is its interleave, and Renderer.convnet gives the same image from the same inputs."""
    from rsd import convnet as rc
    from rsd import graph as rg
    from rsd.frame import Renderer
    monkeypatch.delenv("RSD_CONVNET_FUSED", raising=False)
    monkeypatch.delenv("RSD_NEURALNET_DIR", raising=False)
    cfg = arcade["cfg"]
    W, H = cfg.fb_w, cfg.fb_h
    assert (W, H) == (70, 38)
    layers = CN.make_net("A", 16)
    rc.save_dir(tmp_path / "net", layers)
    text = SCRIPT.read_text()
    assert text.count("'WEIGHTS_DIR'") == 1
    g = rg.load_script(text.replace("'WEIGHTS_DIR'", repr(str(tmp_path / "net"))))["SVAOConvNet"]
    g.set_scene(arcade["gs"].h, arcade["cam"])
    g.compile(W, H)
    g.execute()
    torch.cuda.synchronize()
    guard = g.dict_int("guardBand")
    assert guard == 8
    np_ = lambda name: g.output_tensor(name).cpu().numpy()  # noqa: E731
    ins = [np_(n + ".texOut").reshape(16, 10, 18) for n in ("DeinterleaveBright", "DeinterleaveDark", "DeinterleaveTexture",
                                                            "DeinterleaveDepth")]
    assert [a.dtype for a in ins] == [np.uint8, np.uint8, np.uint8, np.float32]
    # ImageEquation reads the RG8Unorm map: ExtractBright / ExtractDark are its two channels, byte for byte
    ao2 = np_("SVAO.ao").reshape(H, W, 2)
    assert np.array_equal(ins[0], CN.deinterleave(ao2[..., 0])) and np.array_equal(ins[1], CN.deinterleave(ao2[..., 1]))
    assert (ins[0] != ins[1]).any() and len(np.unique(ins[2])) > 5 and len(np.unique(ins[3])) > 20
    # the loader rounds every weight to the 6 significant digits of the reference's shader text
    rounded = [(np.vectorize(lambda v: float("%g" % v))(w).astype(np.float32), np.vectorize(lambda v: float("%g" % v))(b).astype(np.float32))
               for w, b in layers]
    assert any((rw != w).any() for (rw, _), (w, _) in zip(rounded, layers))
    want = CN.run(checker, rounded, ins, W, H, guard, fill=0)
    got = np_("ConvolutionalNet.out").reshape(16, 10, 18)
    m = CN.inside(W, H, 16, guard)
    diff = got != want["out"]
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5], got[diff][:5], want["out"][diff][:5])
    assert len(np.unique(got[m])) > 50
    # the unrounded net gives another image: the rounding is observable
    assert (CN.run(checker, layers, ins, W, H, guard, fill=0)["out"] != want["out"]).any()
    full = np_("InterleaveTexture.texOut").reshape(H, W)
    assert np.array_equal(full, CN.interleave(got, W, H))
    final = np_("AmbientNet.out").reshape(H, W, 4)
    assert np.array_equal(final[..., 0], full) and np.array_equal(final[..., 1], full)
    # Renderer.convnet on the graph's full-size images
    net = rc.ConvNet.from_dir(tmp_path / "net", 16)
    r = Renderer(arcade["scene"], cfg, gpu_scene=arcade["gs"], dev=arcade["dev"])
    image = r.convnet(net, ao2=g.output_tensor("SVAO.ao").reshape(H, W, 2), importance=g.output_tensor("ImageEquation1.out").reshape(H, W),
                      depth=g.output_tensor("ImageEquationLinearDepth.out").reshape(H, W), numerics=1)
    torch.cuda.synchronize()
    assert tuple(image.shape) == (H, W) and image.dtype == torch.float32
    assert np.array_equal(image.cpu().numpy(), full)
    with pytest.raises(ValueError):
        r.convnet(net, ao2=g.output_tensor("SVAO.ao").reshape(H, W, 2)[..., 0])
    g.close()
