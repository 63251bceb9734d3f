"""GPU: rsd_convnet_run against the scalar CPU checker (tests/native/convnet_ref.c, whose known answers and input
conditions tests/test_convnet.py asserts).  Exact numerics compare as floats with no tolerance, on the output and on the
per-layer kernels' stored intermediates; fast numerics stay inside the checker's derived forward error bound.  The
texels outside the scissor keep the sentinel.  RSD_CONVNET_FUSED is read by every rsd_convnet_run, so the tests set it
in this process."""
import ctypes as C

import numpy as np
import pytest

import convnet_checker as CN

pytestmark = pytest.mark.gpu
CASE_IDS = ["%dx%d_S%d_g%d" % c for c in CN.CASES]
F = np.float32
EXACT, FAST = 1, 0
_np_dtype = {CN.FLOAT: np.float32, CN.HALF: np.float16, CN.UNORM: np.uint8}


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return CN.build(tmp_path_factory.mktemp("convnet_ref"))


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def inputs(torch):
    """The synthetic inputs, built once, uploaded once and shared (read-only) by every parameter point."""
    out = {}
    for (W, H, S, g) in CN.CASES:
        s = dict(CN.synthetic(W, H, S))
        s["dev"] = {k: torch.from_numpy(np.array(v)).cuda() for k, v in s.items()}
        out[(W, H, S)] = s
    return out


_nets, _refs = {}, {}


def _net(name, S):
    from rsd import convnet as rc
    if (name, S) not in _nets:
        layers = CN.make_net(name, S)
        _nets[(name, S)] = (layers, rc.ConvNet.from_arrays(layers))
    return _nets[(name, S)]


def _ref(checker, inputs, case, name, precision=CN.FLOAT, clamp=True):
    """The checker's result, computed once per point and shared."""
    key = (case, name, precision, clamp)
    if key not in _refs:
        W, H, S, g = case
        layers, _ = _net(name, S)
        _refs[key] = CN.run(checker, layers, CN.input_list(inputs[(W, H, S)], CN.NETS[name][1][0]), W, H, g, precision, clamp)
    return _refs[key]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _run(torch, net, prm, dev, cin0, stream=None, keys=("bright", "dark", "importance", "depth")):
    """One rsd_convnet_run on fresh sentinel-filled output and scratch; returns (out, scratch) tensors."""
    from rsd import abi
    qshape = tuple(dev[keys[0]].shape)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):  # the fills precede the run
        out = torch.full(qshape, float(CN.SENTINEL), dtype=torch.float32, device="cuda")
        scratch = torch.full((max(net.scratch_bytes(prm), 256),), 0xA5, dtype=torch.uint8, device="cuda")
    ptr = [_p(dev[k]) if c < max(cin0, 2) and k in dev else None for c, k in enumerate(keys)]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else C.c_void_p(stream.cuda_stream)
    abi.check(abi.lib().rsd_convnet_run(net.h, C.byref(prm), *ptr, _p(scratch), _p(out), s), "rsd_convnet_run")
    return out, scratch


def _same(got, want, m):
    diff = m & ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5], got[diff][:5], want[diff][:5])


@pytest.mark.parametrize("fused", ["default", "off"])
@pytest.mark.parametrize("name", sorted(CN.NETS))
@pytest.mark.parametrize("case", CN.CASES, ids=CASE_IDS)
def test_exact_parity(torch, checker, inputs, monkeypatch, case, name, fused):
    """Exact numerics, Float: the output equals the checker as floats on every texel inside the scissor, the sentinel
    remains outside, the inputs are untouched; on the per-layer path the scratch intermediates equal the checker's.
    Net E (radius 12, larger than the layers) takes the path info.fused reports -- the fused kernel, whose LDS rule
    it just fits."""
    from rsd import abi
    W, H, S, g = case
    monkeypatch.setenv("RSD_CONVNET_FUSED", "off") if fused == "off" else monkeypatch.delenv("RSD_CONVNET_FUSED", raising=False)
    layers, net = _net(name, S)
    cin0 = CN.NETS[name][1][0]
    s = inputs[(W, H, S)]
    ref = _ref(checker, inputs, case, name)
    prm = abi.ConvNetParams(W, H, S, g, numerics=EXACT)
    out, scratch = _run(torch, net, prm, s["dev"], cin0)
    torch.cuda.synchronize()
    got, m = out.cpu().numpy(), CN.inside(W, H, S, g)
    assert m.sum() == ref["counters"]["written"] > 0
    _same(got, ref["out"], m)
    assert (got[~m] == CN.SENTINEL).all()
    for k in ("bright", "dark", "importance", "depth"):
        assert np.array_equal(s["dev"][k].cpu().numpy(), s[k])
    if name == "E":
        assert net.fused, "net E's LDS footprint (63040 bytes) fits the fused kernel's 64 KiB"
    if fused == "off" or not net.fused:
        raw = scratch.cpu().numpy()
        for (off, shape), want in zip(net.scratch_layout(prm), ref["inter"]):
            layer = raw[off:off + want.size * 4].view(np.float32).reshape(shape)
            _same(layer, want, np.broadcast_to(m[:, None], shape))
    else:
        assert (scratch.cpu().numpy() == 0xA5).all()  # the fused kernel keeps its intermediates in LDS


@pytest.mark.parametrize("precision", [CN.HALF, CN.UNORM], ids=["half", "unorm"])
@pytest.mark.parametrize("name", sorted(CN.NETS))
@pytest.mark.parametrize("case", CN.CASES, ids=CASE_IDS)
def test_stored_precisions(torch, checker, inputs, monkeypatch, case, name, precision):
    """Half and UNorm intermediates (always the per-layer kernels and the exact arithmetic, whatever numerics asks): the
    stored halves / bytes and the output equal the checker's.  Net B has one layer: no intermediates, the output alone."""
    from rsd import abi
    W, H, S, g = case
    monkeypatch.delenv("RSD_CONVNET_FUSED", raising=False)
    _, net = _net(name, S)
    ref = _ref(checker, inputs, case, name, precision)
    prm = abi.ConvNetParams(W, H, S, g, precision=precision, numerics=FAST)
    out, scratch = _run(torch, net, prm, inputs[(W, H, S)]["dev"], CN.NETS[name][1][0])
    torch.cuda.synchronize()
    got, m, raw = out.cpu().numpy(), CN.inside(W, H, S, g), scratch.cpu().numpy()
    _same(got, ref["out"], m)
    assert (got[~m] == CN.SENTINEL).all()
    dt = _np_dtype[precision]
    for (off, shape), want in zip(net.scratch_layout(prm), ref["inter"]):
        stored = raw[off:off + want.size * np.dtype(dt).itemsize].view(dt).reshape(shape)
        layer = stored.astype(F) / F(255) if precision == CN.UNORM else stored.astype(F)
        _same(layer, want, np.broadcast_to(m[:, None], shape))


@pytest.mark.parametrize("fused", ["default", "off"])
@pytest.mark.parametrize("name", sorted(CN.NETS))
@pytest.mark.parametrize("case", CN.CASES, ids=CASE_IDS)
def test_fast_numerics_within_the_bound(torch, checker, inputs, monkeypatch, case, name, fused):
    """Fast numerics, Float: |fast - exact checker| <= the checker's forward error bound on every texel (derived in
    convnet_ref.c, not tuned), and that bound is far below the clamp range, so the check is not vacuous."""
    from rsd import abi
    W, H, S, g = case
    monkeypatch.setenv("RSD_CONVNET_FUSED", "off") if fused == "off" else monkeypatch.delenv("RSD_CONVNET_FUSED", raising=False)
    _, net = _net(name, S)
    s = inputs[(W, H, S)]
    ref = _ref(checker, inputs, case, name)
    out, _ = _run(torch, net, abi.ConvNetParams(W, H, S, g, numerics=FAST), s["dev"], CN.NETS[name][1][0])
    torch.cuda.synchronize()
    got, m = out.cpu().numpy(), CN.inside(W, H, S, g)
    err = np.abs(got.astype(np.float64) - ref["out"].astype(np.float64))
    print(f"{name} {case} {fused}: max err {err[m].max():.3e}, max bound {ref['bound'][m].max():.3e}")
    assert (err[m] <= ref["bound"][m]).all(), (float(err[m].max()), np.argwhere(m & (err > ref["bound"]))[:5])
    assert (got[~m] == CN.SENTINEL).all()
    clamp_range = np.abs(s["bright"].astype(F) - s["dark"].astype(F))[m] / 255
    assert ref["bound"][m].max() < 0.1 * np.median(clamp_range)


@pytest.mark.parametrize("fused", ["default", "off"])
def test_input_formats_and_unclamped(torch, checker, inputs, monkeypatch, fused):
    """R32Float bright / dark holding the R8 values / 255 give the same result as the bytes (mixed in_texel_bytes);
    clamp_output = 0 passes values outside [dark, bright]; S = 1 runs through CASES[2] in every other test."""
    from rsd import abi
    monkeypatch.setenv("RSD_CONVNET_FUSED", "off") if fused == "off" else monkeypatch.delenv("RSD_CONVNET_FUSED", raising=False)
    case = CN.CASES[0]
    W, H, S, g = case
    _, net = _net("A", S)
    s = inputs[(W, H, S)]
    ref, m = _ref(checker, inputs, case, "A"), CN.inside(W, H, S, g)
    dev = dict(s["dev"])
    dev["bright"] = torch.from_numpy(s["bright"].astype(F) / F(255)).cuda()
    dev["dark"] = torch.from_numpy(s["dark"].astype(F) / F(255)).cuda()
    out, _ = _run(torch, net, abi.ConvNetParams(W, H, S, g, numerics=EXACT, in_texel_bytes=(4, 4, 1, 4)), dev, 4)
    _same(out.cpu().numpy(), ref["out"], m)
    raw = _ref(checker, inputs, case, "A", clamp=False)
    out, _ = _run(torch, net, abi.ConvNetParams(W, H, S, g, numerics=EXACT, clamp_output=False), s["dev"], 4)
    got = out.cpu().numpy()
    _same(got, raw["out"], m)
    b, d = s["bright"].astype(F) / F(255), s["dark"].astype(F) / F(255)
    assert (got[m] > b[m]).any() and (got[m] < d[m]).any()


def test_two_streams_give_identical_bits(torch, inputs, monkeypatch):
    """Two runs on two streams with separate scratch, fused and per-layer, fast and exact: identical bits."""
    from rsd import abi
    W, H, S, g = CN.CASES[0]
    _, net = _net("A", S)
    dev = inputs[(W, H, S)]["dev"]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for fused in ("default", "off"):
        monkeypatch.setenv("RSD_CONVNET_FUSED", "off") if fused == "off" else monkeypatch.delenv("RSD_CONVNET_FUSED", raising=False)
        for numerics in (FAST, EXACT):
            prm = abi.ConvNetParams(W, H, S, g, numerics=numerics)
            a, _ = _run(torch, net, prm, dev, 4, s1)
            b, _ = _run(torch, net, prm, dev, 4, s2)
            torch.cuda.synchronize()
            assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))


def _g(v):
    """A value as the directory loader rounds it: (float)strtod of its "%g" text."""
    return F(float("%g" % float(v)))


def _rounded(layers):
    r = np.vectorize(_g, otypes=[np.float32])
    return [(r(w), None if b is None else r(b)) for w, b in layers]


def test_loader_values(torch, checker, inputs, tmp_path, monkeypatch):
    """What the loaded nets compute (the values are not observable on the host).  A 1 x 1 one-layer net with the weight
    0.1234567 on an input of 1.0, unclamped: 0.123457 through save_dir -> from_dir, 0.1234567 through from_arrays.
    save_dir -> from_dir of net A equals the checker on the "%g"-rounded arrays, not on the raw ones.  A net saved
    without bias files, and one created with bias = None, equal the checker's zero-bias result."""
    from rsd import abi
    from rsd import convnet as rc
    monkeypatch.delenv("RSD_CONVNET_FUSED", raising=False)
    one = [(np.full((1, 1, 1, 1, 1), 0.1234567, F), None)]
    rc.save_dir(tmp_path / "one", one)
    ones = {"bright": torch.ones((1, 4, 5), dtype=torch.float32, device="cuda")}
    prm = abi.ConvNetParams(5, 4, 1, 0, numerics=EXACT, clamp_output=False, in_texel_bytes=(4, 1, 1, 4))
    for net, want in ((rc.ConvNet.from_dir(tmp_path / "one", 1), F(float("0.123457"))), (rc.ConvNet.from_arrays(one), F(0.1234567))):
        out, _ = _run(torch, net, prm, ones, 1)
        got = out.cpu().numpy()
        assert (got == want).all() and got.dtype == np.float32, (got.ravel()[:3], want)
    assert F(float("0.123457")) != F(0.1234567)
    # the round trip of a whole net, with biases
    case = CN.CASES[0]
    W, H, S, g = case
    s, m = inputs[(W, H, S)], CN.inside(W, H, S, g)
    layers = CN.make_net("A", S)
    rc.save_dir(tmp_path / "a", layers)
    prm = abi.ConvNetParams(W, H, S, g, numerics=EXACT)
    out, _ = _run(torch, rc.ConvNet.from_dir(tmp_path / "a", S), prm, s["dev"], 4)
    got = out.cpu().numpy()
    want = CN.run(checker, _rounded(layers), CN.input_list(s), W, H, g)["out"]
    _same(got, want, m)
    assert (got[m] != _ref(checker, inputs, case, "A")["out"][m]).any()  # the rounding is visible
    # no bias: files absent, or bias = None
    case = CN.CASES[2]
    W, H, S, g = case
    s, m = inputs[(W, H, S)], CN.inside(W, H, S, g)
    nobias = [(w, None) for w, _ in CN.make_net("D", S)]
    rc.save_dir(tmp_path / "nobias", nobias)
    assert not list((tmp_path / "nobias").glob("*bias*"))
    prm = abi.ConvNetParams(W, H, S, g, numerics=EXACT)
    for fused in ("default", "off"):
        monkeypatch.setenv("RSD_CONVNET_FUSED", "off") if fused == "off" else monkeypatch.delenv("RSD_CONVNET_FUSED", raising=False)
        for net, arrays in ((rc.ConvNet.from_dir(tmp_path / "nobias", S), _rounded(nobias)), (rc.ConvNet.from_arrays(nobias), nobias)):
            out, _ = _run(torch, net, prm, s["dev"], 4)
            want = CN.run(checker, arrays, CN.input_list(s), W, H, g)
            _same(out.cpu().numpy(), want["out"], m)
    with_bias = _ref(checker, inputs, case, "D")["out"]
    assert (want["out"][m] != with_bias[m]).any()  # the biases matter: zeros are not what net D has
