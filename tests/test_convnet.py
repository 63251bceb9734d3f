"""CPU checks of the ConvolutionalNet feature (rsd_convnet_*, the ConvolutionalNet graph pass, rsd.convnet): the pass is
registered and plans like the reference's, the reference's SAVO_record.py still plans without weights, the C entries
refuse bad arguments without a GPU, the loader reads the reference's file layout with its "%g" rounding, the .npy
parser refuses what it does not read (under ASan + UBSan, in its own process), the scalar checker the GPU tests compare
against (tests/native/convnet_ref.c) gives the answers that can be known in advance, and the inputs of the GPU tests
reach every case of the pass (asserted on the checker alone)."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import convnet_checker as CN
from conftest import ROOT

rsdgraph = pytest.importorskip("rsd.graph")
from rsd import abi  # noqa: E402
from rsd import convnet as rc  # noqa: E402

REF_SCRIPTS = Path("/root/reference/scripts")
needs_gcc = pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
F = np.float32


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return CN.build(tmp_path_factory.mktemp("convnet_ref"))


# ---------------------------------------------------------------------------------- graph

def test_pass_is_builtin():
    assert "ConvolutionalNet" in set(rsdgraph.plugin_types())


def test_planning_a_convnet_chain():
    """DeinterleaveTexture x 4 -> ConvolutionalNet -> InterleaveTexture at 70 x 38: out is R32Float with the size and
    the layer count of bright (ConvolutionalNet.cpp:83-96), and the interleaved image is a full-size R32Float."""
    g = rsdgraph.RenderGraph("net")
    for name in ("B", "D", "I", "Z"):
        g.create_pass(name, "Source", {})
        g.create_pass("De" + name, "DeinterleaveTexture", {})
        g.add_edge(f"{name}.x", f"De{name}.texIn")
    g.create_pass("ConvolutionalNet", "ConvolutionalNet", {})
    g.create_pass("Interleave", "InterleaveTexture", {})
    for name, field in (("B", "bright"), ("D", "dark"), ("I", "importance"), ("Z", "depth")):
        g.add_edge(f"De{name}.texOut", f"ConvolutionalNet.{field}")
    g.add_edge("ConvolutionalNet.out", "Interleave.texIn")
    g.mark_output("Interleave.texOut")
    g.plan(70, 38)
    res = g.resources()
    assert res["ConvolutionalNet.out"] == (18, 10, 16, "R32Float")
    assert res["Interleave.texOut"] == (70, 38, 1, "R32Float")
    order = g.execution_order()
    assert order.index("DeB") < order.index("ConvolutionalNet") < order.index("Interleave")


@pytest.mark.skipif(not REF_SCRIPTS.is_dir(), reason="reference scripts not present (GPU box)")
def test_reference_script_plans_without_weights(monkeypatch):
    """scripts/SAVO_record.py at 2048 x 1208 with no weights directory: the pass constructs, reflects and plans."""
    monkeypatch.delenv("RSD_NEURALNET_DIR", raising=False)
    g = next(iter(rsdgraph.load_script(REF_SCRIPTS / "SAVO_record.py").values()))
    g.plan(1920 + 128, 1080 + 128)
    order, res = g.execution_order(), g.resources()
    assert res["ConvolutionalNet.out"] == (512, 302, 16, "R32Float")
    assert res["InterleaveTexture.texOut"] == (2048, 1208, 1, "R32Float")
    chain = ["DeinterleaveBright", "ConvolutionalNet", "InterleaveTexture", "AmbientNet"]
    assert [order.index(p) for p in chain] == sorted(order.index(p) for p in chain), order


def test_properties(tmp_path, monkeypatch):
    monkeypatch.delenv("RSD_NEURALNET_DIR", raising=False)
    g = rsdgraph.RenderGraph("props")
    g.create_pass("A", "ConvolutionalNet", {})
    g.create_pass("B", "ConvolutionalNet", {"precision": "Half", "clampOutput": False, "numerics": "Exact"})
    g.create_pass("C", "ConvolutionalNet", {"precision": "UNorm"})
    with pytest.raises(abi.RsdError, match="precision"):
        g.create_pass("D", "ConvolutionalNet", {"precision": "Double"})
    with pytest.raises(abi.RsdError, match="numerics"):
        g.create_pass("E", "ConvolutionalNet", {"numerics": "Sloppy"})
    with pytest.raises(abi.RsdError, match="no network"):
        g.create_pass("F", "ConvolutionalNet", {"weights": str(tmp_path / "empty")})
    rc.save_dir(tmp_path / "net", CN.make_net("B", 16))
    g.create_pass("G", "ConvolutionalNet", {"weights": str(tmp_path / "net")})
    monkeypatch.setenv("RSD_NEURALNET_DIR", str(tmp_path / "empty"))  # the default of `weights`
    with pytest.raises(abi.RsdError, match="no network"):
        g.create_pass("H", "ConvolutionalNet", {})


# ---------------------------------------------------------------------------------- ABI

@needs_gcc
def test_abi_mirror(tmp_path):
    """abi.ConvNetLayer / ConvNetInfo / ConvNetParams have the layouts of the header's structs (sizes and offsets
    printed by a C program that includes it); the new entries are exported; the ABI version stays 8."""
    (tmp_path / "s.c").write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "rsd_graph.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
        "sizeof(rsd_convnet_layer), offsetof(rsd_convnet_layer, weights), offsetof(rsd_convnet_layer, bias), "
        "sizeof(rsd_convnet_info), offsetof(rsd_convnet_info, fused), offsetof(rsd_convnet_info, kernel), "
        "offsetof(rsd_convnet_info, channels_out), sizeof(rsd_convnet_params), offsetof(rsd_convnet_params, layers), "
        "offsetof(rsd_convnet_params, numerics), offsetof(rsd_convnet_params, in_texel_bytes));return 0;}\n")
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    sizes = [int(v) for v in subprocess.run([str(tmp_path / "s")], capture_output=True, text=True).stdout.split()]
    Y, I, P = abi.ConvNetLayer, abi.ConvNetInfo, abi.ConvNetParams
    assert sizes == [C.sizeof(Y), Y.weights.offset, Y.bias.offset, C.sizeof(I), I.fused.offset, I.kernel.offset,
                     I.channels_out.offset, C.sizeof(P), P.layers.offset, P.numerics.offset, P.in_texel_bytes.offset] == \
        [32, 16, 24, 112, 12, 16, 80, 44, 12, 24, 28]
    p = P(70, 38)
    assert (p.width, p.height, p.guard_band, p.layers, p.precision, p.clamp_output, p.numerics, list(p.in_texel_bytes)) == \
        (70, 38, 0, 16, 0, 1, 0, [1, 1, 1, 4])
    L = abi.lib()
    for name in ("rsd_convnet_create", "rsd_convnet_load_dir", "rsd_convnet_release", "rsd_convnet_get_info",
                 "rsd_convnet_scratch_bytes", "rsd_convnet_run"):
        assert getattr(L, name) is not None and name in abi.GRAPH_EXPORTS + abi.GRAPH_SIZE_EXPORTS
    assert L.rsd_abi_version() == 8


def test_arguments_are_checked():
    """rsd_convnet_run refuses null pointers, an empty extent and a texel size outside {1, 4} (status 1), a layer count
    that is not the net's, a bad precision (status 2) -- on the host, before any GPU work: the pointers are never
    dereferenced.  Fast numerics with Half / UNorm is accepted: those precisions always run the exact arithmetic."""
    L = abi.lib()
    net = rc.ConvNet.from_arrays(CN.make_net("A", 16))
    assert (net.layers, net.slices, net.radius, net.kernel, net.channels_in, net.channels_out) == \
        (3, 16, 3, [3, 3, 3], [4, 6, 5], [6, 5, 1])
    p = C.c_void_p(1 << 20)
    P = abi.ConvNetParams
    ok = dict(net=net.h, prm=P(70, 38), b=p, d=p, i=p, z=p, s=p, o=p)

    def run(**kw):
        a = {**ok, **kw}
        return L.rsd_convnet_run(a["net"], C.byref(a["prm"]) if a["prm"] is not None else None, a["b"], a["d"], a["i"],
                                 a["z"], a["s"], a["o"], None)

    bad = [dict(net=None), dict(prm=None), dict(b=None), dict(d=None), dict(i=None), dict(z=None), dict(s=None),
           dict(o=None), dict(prm=P(0, 38)), dict(prm=P(70, 0)), dict(prm=P(70, 38, in_texel_bytes=(2, 1, 1, 4))),
           dict(prm=P(70, 38, in_texel_bytes=(1, 1, 1, 0))), dict(prm=P(70, 38, numerics=2))]
    for b in bad:
        assert run(**b) == abi.ERR_INVALID_ARG, b
        assert b"rsd_convnet_run" in L.rsd_last_error(), b
    for layers in (0, 1, 4, 17):
        assert run(prm=P(70, 38, layers=layers)) == abi.ERR_UNSUPPORTED, layers
        assert b"layers" in L.rsd_last_error()
    assert run(prm=P(70, 38, precision=3)) == abi.ERR_UNSUPPORTED and b"precision" in L.rsd_last_error()
    # a guard band that leaves nothing inside the scissor draws nothing (and touches nothing), also with fast + Half
    assert run(prm=P(70, 38, guard_band=40)) == 0
    assert run(prm=P(70, 38, guard_band=40, precision="Half", numerics=0)) == 0
    # inputs beyond Cin_0 may be NULL: net C reads three channels
    netc = rc.ConvNet.from_arrays(CN.make_net("C", 16))
    assert L.rsd_convnet_run(netc.h, C.byref(P(70, 38, guard_band=40)), p, p, p, None, p, p, None) == 0
    assert L.rsd_convnet_run(netc.h, C.byref(P(70, 38, guard_band=40)), p, p, None, None, p, p, None) == abi.ERR_INVALID_ARG
    # scratch: one 256-byte-aligned block of [S][Cout][qh][qw] per layer but the last
    assert net.scratch_bytes(P(70, 38)) == 16 * 6 * 180 * 4 + 16 * 5 * 180 * 4
    assert net.scratch_bytes(P(70, 38, precision="UNorm")) == sum((16 * c * 180 + 255) // 256 * 256 for c in (6, 5))
    assert [o for o, _ in net.scratch_layout(P(70, 38))] == [0, 16 * 6 * 180 * 4]
    info = abi.ConvNetInfo()
    assert L.rsd_convnet_get_info(None, C.byref(info)) == abi.ERR_INVALID_ARG
    assert L.rsd_convnet_get_info(net.h, None) == abi.ERR_INVALID_ARG
    h = C.c_void_p()
    assert L.rsd_convnet_create(None, 1, 16, C.byref(h)) == abi.ERR_INVALID_ARG
    assert L.rsd_convnet_load_dir(None, 16, C.byref(h)) == abi.ERR_INVALID_ARG


def test_net_shapes_are_checked():
    w = lambda k, ci, co, s=16: (np.zeros((s, k, k, ci, co), F), None)  # noqa: E731
    for layers, what in (([w(3, 5, 1)], "at most 4"), ([w(3, 4, 6), w(3, 5, 1)], "reads 5"), ([w(3, 4, 33), w(3, 33, 1)], "1..32"),
                         ([w(3, 4, 4)] * 9, "1..8 layers"), ([w(3, 4, 1, 4)], "slices")):
        with pytest.raises(abi.RsdError, match=what) as e:
            rc.ConvNet.from_arrays(layers)
        assert e.value.status == abi.ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="non-square"):
        rc.ConvNet.from_arrays([(np.zeros((16, 3, 2, 4, 1), F), None)])
    e = rc.ConvNet.from_arrays(CN.make_net("E", 16))
    assert e.radius == 12 and e.kernel == [7] * 4
    assert rc.ConvNet.from_arrays(CN.make_net("D", 1)).radius == 2


# ---------------------------------------------------------------------------------- loader

def test_loader_reads_the_file_layout(tmp_path):
    """save_dir writes the reference's file names and load_dir reads them back into a net of the saved shape; a
    directory without bias files loads.  A loaded net's values are not observable on the host: that 0.1234567 loads
    as float("0.123457") while from_arrays keeps it, that a whole net round trips and that a missing bias is zeros is
    asserted on what the nets compute, in tests/test_gpu_convnet.py::test_loader_values."""
    layers = CN.make_net("A", 16)
    rc.save_dir(tmp_path / "a", layers)
    assert (tmp_path / "a" / "15_weight_2.npy").exists() and (tmp_path / "a" / "0_bias_0.npy").exists()
    net = rc.ConvNet.from_dir(tmp_path / "a", 16)
    assert (net.layers, net.slices, net.kernel, net.channels_in, net.channels_out) == (3, 16, [3] * 3, [4, 6, 5], [6, 5, 1])
    assert np.array_equal(np.load(tmp_path / "a" / "3_weight_1.npy"), layers[1][0][3])
    # a missing bias file loads; a plain image is slice count 1
    rc.save_dir(tmp_path / "nobias", [(w, None) for w, _ in CN.make_net("D", 1)])
    assert not (tmp_path / "nobias" / "0_bias_0.npy").exists()
    assert rc.ConvNet.from_dir(tmp_path / "nobias", 1).layers == 2


def test_loader_refuses(tmp_path):
    L = abi.lib()

    def refused(d, slices, status, what):
        with pytest.raises(abi.RsdError, match=what) as e:
            rc.ConvNet.from_dir(d, slices)
        assert e.value.status == status, L.rsd_last_error()

    refused(tmp_path / "nothing", 16, abi.ERR_INVALID_ARG, "no network")
    # a slice with another layer count
    rc.save_dir(tmp_path / "count", CN.make_net("A", 16))
    (tmp_path / "count" / "7_weight_2.npy").unlink()
    refused(tmp_path / "count", 16, abi.ERR_UNSUPPORTED, "layer count")
    # a slice with other channel counts
    rc.save_dir(tmp_path / "shape", CN.make_net("A", 16))
    np.save(tmp_path / "shape" / "5_weight_1.npy", np.zeros((3, 3, 6, 4), F))
    refused(tmp_path / "shape", 16, abi.ERR_UNSUPPORTED, "slice 0")
    # non-square kernels
    (tmp_path / "rect").mkdir()
    np.save(tmp_path / "rect" / "0_weight_0.npy", np.zeros((3, 2, 4, 1), F))
    refused(tmp_path / "rect", 1, abi.ERR_UNSUPPORTED, "non-square")
    # float64, Fortran order, truncated
    for name, array in (("f8", np.zeros((1, 1, 4, 1), np.float64)), ("fortran", np.asfortranarray(np.ones((2, 2, 4, 1), F)))):
        (tmp_path / name).mkdir()
        np.save(tmp_path / name / "0_weight_0.npy", array)
    refused(tmp_path / "f8", 1, abi.ERR_INVALID_ARG, "float32")
    refused(tmp_path / "fortran", 1, abi.ERR_INVALID_ARG, "Fortran")
    (tmp_path / "cut").mkdir()
    np.save(tmp_path / "cut" / "0_weight_0.npy", np.ones((3, 3, 4, 1), F))
    data = (tmp_path / "cut" / "0_weight_0.npy").read_bytes()
    (tmp_path / "cut" / "0_weight_0.npy").write_bytes(data[:-10])
    refused(tmp_path / "cut", 1, abi.ERR_INVALID_ARG, "truncated")
    (tmp_path / "cut" / "0_weight_0.npy").write_bytes(data[:40])
    refused(tmp_path / "cut", 1, abi.ERR_INVALID_ARG, "truncated header")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_npy_parser_under_sanitizers(tmp_path):
    """csrc/host/npy.h over good and malformed files, in a stand-alone program built with ASan + UBSan."""
    exe = tmp_path / "check_npy"
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "ray-traced-stochastic-depth-map_amd" / "csrc"),
                    str(ROOT / "tests" / "native" / "check_npy.cpp"), "-o", str(exe)], check=True)
    good = np.arange(3 * 3 * 4 * 2, dtype=F).reshape(3, 3, 4, 2)
    np.save(tmp_path / "good.npy", good)
    np.save(tmp_path / "bias.npy", np.array([0.5, -1.5], F))
    np.save(tmp_path / "f8.npy", good.astype(np.float64))
    np.save(tmp_path / "be.npy", good.astype(">f4"))
    np.save(tmp_path / "fortran.npy", np.asfortranarray(good))
    np.save(tmp_path / "scalar.npy", F(2.0))
    raw = (tmp_path / "good.npy").read_bytes()
    header_len = int.from_bytes(raw[8:10], "little")
    (tmp_path / "cut_payload.npy").write_bytes(raw[:-4])
    (tmp_path / "cut_header.npy").write_bytes(raw[:30])
    (tmp_path / "cut_preamble.npy").write_bytes(raw[:7])
    (tmp_path / "magic.npy").write_bytes(b"NOTNUMPY" + raw[8:])
    (tmp_path / "long.npy").write_bytes(raw + b"\0" * 8)
    header = raw[10:10 + header_len].decode()
    assert "(3, 3, 4, 2)" in header
    huge = header.replace("(3, 3, 4, 2)", "(4294967296, 4294967296, 4, 2)")  # 2^64 x 8 values
    (tmp_path / "overflow.npy").write_bytes(raw[:8] + len(huge).to_bytes(2, "little") + huge.encode() + raw[10 + header_len:])
    v2 = raw[:6] + b"\x02\x00" + header_len.to_bytes(4, "little") + raw[10:]
    (tmp_path / "v2.npy").write_bytes(v2)
    (tmp_path / "v3.npy").write_bytes(raw[:6] + b"\x03\x00" + header_len.to_bytes(4, "little") + raw[10:])
    names = ["good", "bias", "v2", "scalar", "f8", "be", "fortran", "cut_payload", "cut_header", "cut_preamble", "magic",
             "long", "overflow", "v3", "missing"]
    r = subprocess.run([str(exe)] + [str(tmp_path / f"{n}.npy") for n in names], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = dict(zip(names, r.stdout.splitlines()))
    assert len(lines) == len(names), r.stdout
    assert lines["good"] == f"ok 4 3 3 4 2 {float(good.sum()):.9g}"
    assert lines["bias"] == "ok 1 2 -1" and lines["v2"] == lines["good"] and lines["scalar"] == "ok 0 2"
    for name, what in (("f8", "float32"), ("be", "'>f4'"), ("fortran", "Fortran"), ("cut_payload", "truncated"),
                       ("cut_header", "truncated header"), ("cut_preamble", "magic"), ("magic", "magic"),
                       ("long", "payload bytes"), ("overflow", "overflows"), ("v3", "version 3.0"), ("missing", "cannot open")):
        assert lines[name].startswith("error ") and what in lines[name], (name, lines[name])


# ---------------------------------------------------------------------------------- the checker, pinned

def _img(values):
    return np.ascontiguousarray(np.asarray(values, F)[None])


def _one(k, cin, cout, taps):
    """One slice, one layer of zeros with w[a][b][c][co] = v for (a, b, c, co, v) in taps; no bias."""
    w = np.zeros((1, k, k, cin, cout), F)
    for a, b, c, co, v in taps:
        w[0, a, b, c, co] = v
    return (w, None)


@needs_gcc
def test_identity_and_clamp(checker):
    rng = np.random.default_rng(1)
    bright = rng.uniform(0.4, 0.9, (1, 7, 9)).astype(F)
    dark = (bright * F(0.5)).astype(F)
    r = CN.run(checker, [_one(1, 2, 1, [(0, 0, 0, 0, 1.0)])], [bright, dark], 9, 7)
    assert np.array_equal(r["out"], bright) and r["counters"]["written"] == 63 and r["counters"]["clamp_inside"] == 63
    # 3 x bright is above bright, -bright below dark; without the clamp both pass
    for gain, want, counter in ((3.0, bright, "clamp_high"), (-1.0, dark, "clamp_low")):
        layer = [_one(1, 2, 1, [(0, 0, 0, 0, gain)])]
        r = CN.run(checker, layer, [bright, dark], 9, 7)
        assert np.array_equal(r["out"], want) and r["counters"][counter] == 63
        assert np.array_equal(CN.run(checker, layer, [bright, dark], 9, 7, clamp_output=False)["out"], F(gain) * bright)
    # dark > bright gives bright; R8Unorm inputs read byte / 255
    b8, d8 = np.full((1, 4, 4), 90, np.uint8), np.full((1, 4, 4), 250, np.uint8)
    r = CN.run(checker, [_one(1, 2, 1, [(0, 0, 1, 0, 0.5)])], [b8, d8], 4, 4)
    assert np.array_equal(r["out"], np.full((1, 4, 4), F(90) / F(255)))
    r = CN.run(checker, [_one(1, 2, 1, [(0, 0, 1, 0, 0.5)])], [d8, b8], 4, 4)
    assert np.array_equal(r["out"], np.full((1, 4, 4), F(90) / F(255)))  # half of dark is below dark


@needs_gcc
def test_axis_order_and_zero_outside_the_image(checker):
    """A 3 x 3 kernel whose only 1 is at a = 0, b = 1 gives out(x, y) = in(x - 1, y), and 0 in column 0: axis 0 of the
    weights is the x offset, and a tap outside the image reads 0.  An even kernel's taps are at -1 and 0."""
    img = np.arange(1, 36, dtype=F).reshape(1, 5, 7)
    r = CN.run(checker, [_one(3, 1, 1, [(0, 1, 0, 0, 1.0)])], [img, img], 7, 5, clamp_output=False)
    assert np.array_equal(r["out"][0, :, 1:], img[0, :, :-1]) and (r["out"][0, :, 0] == 0).all()
    r = CN.run(checker, [_one(3, 1, 1, [(1, 2, 0, 0, 1.0)])], [img, img], 7, 5, clamp_output=False)
    assert np.array_equal(r["out"][0, :-1], img[0, 1:]) and (r["out"][0, -1] == 0).all()
    r = CN.run(checker, [_one(2, 1, 1, [(0, 1, 0, 0, 1.0)])], [img, img], 7, 5, clamp_output=False)  # (x - 1, y + 0)
    assert np.array_equal(r["out"][0, :, 1:], img[0, :, :-1]) and (r["out"][0, :, 0] == 0).all()
    # all ones on a constant image counts the taps inside the image: 4 in the corners, 6 on the edges, 9 inside
    ones = np.ones((1, 5, 7), F)
    r = CN.run(checker, [(np.ones((1, 3, 3, 1, 1), F), None)], [ones, ones], 7, 5, clamp_output=False)
    want = np.full((5, 7), 9, F)
    want[0, :] = want[-1, :] = want[:, 0] = want[:, -1] = 6
    want[0, 0] = want[0, -1] = want[-1, 0] = want[-1, -1] = 4
    assert np.array_equal(r["out"][0], want)
    assert r["counters"]["tap_outside_image"] == int((9 - want).sum())


@needs_gcc
def test_relu_scissor_and_channel_zero(checker):
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, (1, 9, 11)).astype(F)
    # ReLU removes the negatives of layer 0; layer 1 copies them out
    net = [_one(1, 1, 1, [(0, 0, 0, 0, 1.0)]), _one(1, 1, 1, [(0, 0, 0, 0, 1.0)])]
    r = CN.run(checker, net, [x, x], 11, 9, clamp_output=False)
    assert np.array_equal(r["out"], np.maximum(x, 0)) and np.array_equal(r["inter"][0][:, 0], np.maximum(x, 0))
    assert r["counters"]["relu_clipped"] == int((x < 0).sum()) and r["counters"]["relu_passed"] == int((x > 0).sum())
    # next to the scissor (plain image, guard band 2): the intermediates outside it are 0 and read 0 -- an all-ones
    # second layer sums only the inside part of its window, although the inputs outside are not 0 --, and the output
    # keeps the sentinel outside
    ones = np.ones((1, 9, 11), F)
    net = [_one(1, 1, 1, [(0, 0, 0, 0, 1.0)]), (np.ones((1, 3, 3, 1, 1), F), None)]
    r = CN.run(checker, net, [ones, ones], 11, 9, guard_band=2, clamp_output=False)
    m = CN.inside(11, 9, 1, 2)
    assert (r["out"][~m] == CN.SENTINEL).all() and (r["inter"][0][:, 0][~m] == 0).all() and (r["inter"][0][:, 0][m] == 1).all()
    want = np.full((5, 7), 9, F)
    want[0, :] = want[-1, :] = want[:, 0] = want[:, -1] = 6
    want[0, 0] = want[0, -1] = want[-1, 0] = want[-1, -1] = 4
    assert np.array_equal(r["out"][0, 2:-2, 2:-2], want) and r["counters"]["tap_outside_scissor"] == int((9 - want).sum())
    # a first layer next to the scissor still reads the real inputs outside it
    r = CN.run(checker, [(np.ones((1, 3, 3, 1, 1), F), None)], [ones, ones], 11, 9, guard_band=2, clamp_output=False)
    assert (r["out"][m] == 9).all()
    # only channel 0 of the last layer is output: changing channel 1's weights changes nothing
    syn = CN.synthetic(70, 38, 16)
    netc = CN.make_net("C", 16)
    a = CN.run(checker, netc, CN.input_list(syn, 3), 70, 38, 8)["out"]
    netc[-1][0][..., 1] += F(1)
    netc[-1][1][:, 1] -= F(3)
    assert np.array_equal(a, CN.run(checker, netc, CN.input_list(syn, 3), 70, 38, 8)["out"])


@needs_gcc
def test_precisions_change_the_result(checker):
    syn, net = CN.synthetic(70, 38, 16), CN.make_net("A", 16)
    f = CN.run(checker, net, CN.input_list(syn), 70, 38, 8, CN.FLOAT)
    h = CN.run(checker, net, CN.input_list(syn), 70, 38, 8, CN.HALF)
    u = CN.run(checker, net, CN.input_list(syn), 70, 38, 8, CN.UNORM)
    m = CN.inside(70, 38, 16, 8)
    assert (f["out"][m] != h["out"][m]).any() and (f["out"][m] != u["out"][m]).any() and (h["out"][m] != u["out"][m]).any()
    # the stored formats: halves are halves, unorm bytes / 255 in [0, 1]
    assert np.array_equal(h["inter"][0], h["inter"][0].astype(np.float16).astype(F))
    assert not np.array_equal(f["inter"][0], f["inter"][0].astype(np.float16).astype(F))
    assert np.array_equal(u["inter"][0], np.round(u["inter"][0] * 255).astype(F) / F(255)) and u["inter"][0].max() <= 1
    # binary16 rounding of the checker against numpy's, over every class of value
    vals = np.concatenate([np.random.default_rng(3).uniform(0, 70000, 2000), np.random.default_rng(4).uniform(0, 1e-4, 2000),
                           [0, 65504, 65519.9, 65520, 6e-8, 2.98e-8, 2.9802322e-8, 1 + 2 ** -11, 1 + 3 * 2 ** -11]]).astype(F)
    one = [_one(1, 1, 1, [(0, 0, 0, 0, 1.0)])] * 2
    img = vals.reshape(1, 1, -1)
    got = CN.run(checker, one, [img, img], vals.size, 1, precision=CN.HALF, clamp_output=False)["out"]
    with np.errstate(over="ignore"):
        assert np.array_equal(got.ravel(), vals.astype(np.float16).astype(F))


# ---------------------------------------------------------------------------------- input conditions

@needs_gcc
@pytest.mark.parametrize("case", CN.CASES, ids=lambda c: "x".join(map(str, c)))
def test_inputs_reach_every_case(checker, case):
    """On every case and net A every counter of the checker is at least 1, with one exception that geometry forces: a
    first-layer tap leaves the image only where the layer's reach K / 2 exceeds the scissor, and net A reaches 1 texel
    against scissors of 2 (case 1) and 3 (case 3).  There the counter is asserted to be 0; it is at least 1 on case 2
    (no guard band) and on case 1 with net E (reach 3), and no net of the set reaches beyond case 3's scissor of 3.
    On case 2 the scissor is the image, so the taps outside the scissor are those of the later layers outside the
    image.  The error bound of the fast-numerics test is far below the clamp range."""
    W, H, S, guard = case
    syn = CN.synthetic(W, H, S)
    r = CN.run(checker, CN.make_net("A", S), CN.input_list(syn), W, H, guard)
    for name in CN.COUNTERS:
        if name == "tap_outside_image" and CN.scissor(guard, S) >= CN.NETS["A"][0] // 2:
            assert r["counters"][name] == 0
        else:
            assert r["counters"][name] >= 1, (name, r["counters"])
    if case == CN.CASES[0]:
        e = CN.run(checker, CN.make_net("E", S), CN.input_list(syn), W, H, guard)
        assert e["counters"]["tap_outside_image"] >= 1 and e["counters"]["tap_outside_scissor"] >= 1
    m = CN.inside(W, H, S, guard)
    assert r["counters"]["written"] == int(m.sum()) and (r["out"][~m] == CN.SENTINEL).all()
    clamp_range = np.abs(syn["bright"].astype(F) - syn["dark"].astype(F))[m] / 255
    assert 0 < r["bound"][m].max() < 0.1 * np.median(clamp_range)
    assert (syn["dark"] > syn["bright"]).any() and (syn["dark"] < syn["bright"]).any()


@needs_gcc
def test_nets_differ(checker):
    W, H, S, guard = CN.CASES[0]
    syn = CN.synthetic(W, H, S)
    m = CN.inside(W, H, S, guard)
    outs = {n: CN.run(checker, CN.make_net(n, S), CN.input_list(syn, CN.NETS[n][1][0]), W, H, guard)["out"][m] for n in CN.NETS}
    names = sorted(outs)
    for i, a in enumerate(names):
        assert len(np.unique(outs[a])) > 50, a
        for b in names[i + 1:]:
            assert (outs[a] != outs[b]).mean() > 0.2, (a, b)
