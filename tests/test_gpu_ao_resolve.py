"""GPU: rsd_ao_guided_blur, rsd_ao_variance_fix and rsd_ao_first_channel against the scalar CPU checker
(tests/native/ao_resolve_ref.c, whose known answers and input conditions tests/test_ao_resolve.py asserts).  Every
comparison is on the R8Unorm / RGBA8Unorm bytes, bit for bit; the texels outside the scissor keep the sentinel."""
import ctypes as C

import numpy as np
import pytest

import ao_resolve_checker as AR

pytestmark = pytest.mark.gpu
CASE_IDS = ["%dx%d_L%d_g%d" % c for c in AR.CASES]


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return AR.build(tmp_path_factory.mktemp("ao_resolve_ref"))


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def inputs(torch):
    """The synthetic inputs, built once, uploaded once and shared (read-only) by every parameter point."""
    out = {}
    for (W, H, L, g) in AR.CASES:
        if (W, H, L) not in out:
            s = AR.synthetic(W, H, L)
            s["dev"] = {k: torch.from_numpy(np.array(s[k])).cuda() for k in ("ao2", "bright", "dark", "depth")}
            out[(W, H, L)] = s
    return out


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("source", ["ao2", "bright"], ids=["rg8", "r8"])
@pytest.mark.parametrize("local_deviation", [True, False], ids=["ldev", "adev"])
@pytest.mark.parametrize("radius", AR.RADII)
@pytest.mark.parametrize("case", AR.CASES, ids=CASE_IDS)
def test_guided_blur_parity(torch, checker, inputs, case, radius, local_deviation, source):
    """rsd_ao_guided_blur equals the checker byte for byte, in the output and in the ping-pong image; both keep the
    sentinel on every texel outside the scissor; the inputs are untouched."""
    from rsd import abi
    W, H, L, g = case
    s = inputs[(W, H, L)]
    d = s["dev"]
    shape = tuple(s["depth"].shape)
    ping = torch.full(shape + (4,), AR.SENTINEL, dtype=torch.uint8, device="cuda")
    dst = torch.full(shape, AR.SENTINEL, dtype=torch.uint8, device="cuda")
    prm = abi.AOGuidedBlurParams(W, H, L, 2 if source == "ao2" else 1, radius, local_deviation, g)
    abi.check(abi.lib().rsd_ao_guided_blur(C.byref(prm), _p(d[source]), _p(d["depth"]), _p(ping), _p(dst),
                                           _stream(torch)), "rsd_ao_guided_blur")
    torch.cuda.synchronize()
    got, got_ping = dst.cpu().numpy(), ping.cpu().numpy()
    want, want_ping, n = AR.guided_blur(checker, s[source], s["depth"], W, H, g, radius, local_deviation)
    m = AR.inside(W, H, L, g)
    assert n["written"] == m.sum() > 0
    diff_ping = (got_ping != want_ping).any(-1)
    assert not diff_ping.any(), (int(diff_ping.sum()), np.argwhere(diff_ping)[:5], got_ping[diff_ping][:5],
                                 want_ping[diff_ping][:5])
    diff = got != want
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5], got[diff][:5], want[diff][:5])
    assert (got[~m] == AR.SENTINEL).all() and (got_ping[~m] == AR.SENTINEL).all()
    for k in (source, "depth"):
        assert np.array_equal(d[k].cpu().numpy().view(np.uint8), np.asarray(s[k]).view(np.uint8)), k


@pytest.mark.parametrize("case", AR.CASES, ids=CASE_IDS)
def test_variance_fix_parity(torch, checker, inputs, case):
    """rsd_ao_variance_fix equals the checker byte for byte at the same sizes (guard band 6 puts uvMin and uvMax
    between texel centres, where the bilinear rule decides); the sentinel stays outside the scissor."""
    from rsd import abi
    W, H, L, g = case
    s = inputs[(W, H, L)]
    d = s["dev"]
    dst = torch.full(tuple(s["depth"].shape), AR.SENTINEL, dtype=torch.uint8, device="cuda")
    prm = abi.AOVarianceFixParams(W, H, L, g)
    abi.check(abi.lib().rsd_ao_variance_fix(C.byref(prm), _p(d["bright"]), _p(d["dark"]), _p(d["depth"]), _p(dst),
                                            _stream(torch)), "rsd_ao_variance_fix")
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    want, n = AR.variance_fix(checker, s["bright"], s["dark"], s["depth"], W, H, g)
    m = AR.inside(W, H, L, g)
    diff = got != want
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5], got[diff][:5], want[diff][:5])
    assert n["written"] == m.sum() > 0 and (got[~m] == AR.SENTINEL).all()
    assert len(np.unique(got[m])) > 30


def test_plain_image_with_a_guard_band(torch, checker, inputs):
    """One layer with a guard band: the scissor is the guard band itself (70 x 38, guard band 6)."""
    from rsd import abi
    W, H, g = 70, 38, 6
    s = AR.synthetic(W, H, 1)
    src, z = torch.from_numpy(np.array(s["ao2"])).cuda(), torch.from_numpy(np.array(s["depth"])).cuda()
    ping = torch.full((1, H, W, 4), AR.SENTINEL, dtype=torch.uint8, device="cuda")
    dst = torch.full((1, H, W), AR.SENTINEL, dtype=torch.uint8, device="cuda")
    prm = abi.AOGuidedBlurParams(W, H, 1, 2, 4, True, g)
    abi.check(abi.lib().rsd_ao_guided_blur(C.byref(prm), _p(src), _p(z), _p(ping), _p(dst), _stream(torch)),
              "rsd_ao_guided_blur")
    torch.cuda.synchronize()
    want, want_ping, n = AR.guided_blur(checker, s["ao2"], s["depth"], W, H, g, 4, True)
    assert n["written"] == (W - 12) * (H - 12)
    assert np.array_equal(dst.cpu().numpy(), want) and np.array_equal(ping.cpu().numpy(), want_ping)


def test_an_infinite_depth_meets_the_min(torch, checker, inputs):
    """A patch of depth +inf (tests/test_ao_resolve.py: inf / inf is NaN, min(NaN, 1) is 1, the weight 0 and the texel
    takes the fallback; AOVarianceFix's saturate(NaN) is 0, the weight 1): both entries equal the checker."""
    from rsd import abi
    W, H, L, g = 70, 38, 16, 8
    s = inputs[(W, H, L)]
    z = np.array(s["depth"])
    z[:, 4:7, 5:9] = np.inf
    dz = torch.from_numpy(z).cuda()
    d = s["dev"]
    ping = torch.full(z.shape + (4,), AR.SENTINEL, dtype=torch.uint8, device="cuda")
    dst = torch.full(z.shape, AR.SENTINEL, dtype=torch.uint8, device="cuda")
    prm = abi.AOGuidedBlurParams(W, H, L, 2, 2, True, g)
    abi.check(abi.lib().rsd_ao_guided_blur(C.byref(prm), _p(d["ao2"]), _p(dz), _p(ping), _p(dst), _stream(torch)),
              "rsd_ao_guided_blur")
    fix = torch.full(z.shape, AR.SENTINEL, dtype=torch.uint8, device="cuda")
    vp = abi.AOVarianceFixParams(W, H, L, g)
    abi.check(abi.lib().rsd_ao_variance_fix(C.byref(vp), _p(d["bright"]), _p(d["dark"]), _p(dz), _p(fix), _stream(torch)),
              "rsd_ao_variance_fix")
    torch.cuda.synchronize()
    want, want_ping, n = AR.guided_blur(checker, s["ao2"], z, W, H, g, 2, True)
    assert n["fallback_x"] >= 16 * 12
    assert np.array_equal(ping.cpu().numpy(), want_ping) and np.array_equal(dst.cpu().numpy(), want)
    assert np.array_equal(dst.cpu().numpy()[:, 4:7, 5:9], np.asarray(s["bright"])[:, 4:7, 5:9])
    assert np.array_equal(fix.cpu().numpy(), AR.variance_fix(checker, s["bright"], s["dark"], z, W, H, g)[0])


def test_an_empty_scissor_draws_nothing(torch, inputs):
    from rsd import abi
    s = inputs[(70, 38, 16)]
    d = s["dev"]
    shape = tuple(s["depth"].shape)
    ping = torch.full(shape + (4,), AR.SENTINEL, dtype=torch.uint8, device="cuda")
    dst = torch.full(shape, AR.SENTINEL, dtype=torch.uint8, device="cuda")
    prm = abi.AOGuidedBlurParams(70, 38, 16, 2, 2, True, 20)  # scissor 5 on 18 x 10 layers
    abi.check(abi.lib().rsd_ao_guided_blur(C.byref(prm), _p(d["ao2"]), _p(d["depth"]), _p(ping), _p(dst),
                                           _stream(torch)), "rsd_ao_guided_blur")
    torch.cuda.synchronize()
    assert (dst == AR.SENTINEL).all() and (ping == AR.SENTINEL).all()


@pytest.mark.parametrize("texel", [1, 2])
def test_first_channel(torch, texel):
    """rsd_ao_first_channel, the disabled pass's blit: byte 0 of every texel, all layers, no scissor."""
    from rsd import abi
    rng = np.random.default_rng(texel)
    src = rng.integers(0, 256, (16, 10, 18, texel), dtype=np.uint8)
    dsrc = torch.from_numpy(src).cuda()
    dst = torch.full((16, 10, 18), AR.SENTINEL, dtype=torch.uint8, device="cuda")
    abi.check(abi.lib().rsd_ao_first_channel(_p(dsrc), texel, 16 * 10 * 18, _p(dst), _stream(torch)),
              "rsd_ao_first_channel")
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), src[..., 0])
