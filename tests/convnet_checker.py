"""The CPU checker of the ConvolutionalNet tests (tests/native/convnet_ref.c): a scalar restatement of the pass that
shares no code with csrc/convnet.hip, the seeded nets A-E and the synthetic inputs every test file runs.  Shared by
tests/test_convnet.py (known answers, input conditions), tests/test_gpu_convnet.py and tests/test_gpu_graph_convnet.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from hbao_checker import deinterleave, interleave  # noqa: F401  (DeinterleaveTexture / InterleaveTexture on the host)

HERE = Path(__file__).resolve().parent
F = np.float32
SENTINEL = F(-7.5)  # what the output holds before a run: no clamped result equals it
COUNTERS = ["written", "relu_clipped", "relu_passed", "clamp_low", "clamp_high", "clamp_inside", "tap_outside_image",
            "tap_outside_scissor"]
FLOAT, HALF, UNORM = 0, 1, 2

# (width, height, slices, guard band) of the full-size frame: 18 x 10 layers with scissor 8 / 4 = 2; ragged 10 x 6
# layers (37 x 23 is no multiple of 4) without a guard band; one plain 21 x 13 image with scissor 3
CASES = [(70, 38, 16, 8), (37, 23, 16, 0), (21, 13, 1, 3)]

# name -> (kernel size, channel counts): A has channel counts that are no multiples of 4; B is one 1 x 1 layer; C reads
# 3 inputs and ends in two channels (only channel 0 is output); D has an even kernel (taps at -1 and 0); E's radius 12
# exceeds the layers: tile halo and image edge at once
NETS = {"A": (3, [4, 6, 5, 1]), "B": (1, [4, 1]), "C": (5, [3, 8, 2]), "D": (2, [4, 4, 1]), "E": (7, [4, 4, 4, 4, 1])}

# spread of the weights, x 2.5 / sqrt(fan-in): the worst-case error bound grows with (sum |w|) ^ (layers - 1), and E's
# four 7 x 7 layers need a smaller spread for the bound to stay far below the clamp range
NET_SCALE = {"E": 0.2}

_lib = None


def build(out_dir):
    """Compile the checker (once per process): gcc, no contraction, SSE arithmetic."""
    global _lib
    if _lib is None:
        so = Path(out_dir) / "libconvnet_ref.so"
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-msse2", "-mfpmath=sse", "-shared", "-fPIC", "-o", str(so),
                        str(HERE / "native" / "convnet_ref.c"), "-lm"], check=True)
        L = C.CDLL(str(so))
        vp, i = C.c_void_p, C.c_int
        L.convnet_ref.restype = None
        L.convnet_ref.argtypes = [i, i, vp, vp, vp, vp, vp, i, i, i, vp, vp, i, i, vp, vp, vp, vp]
        _lib = L
    return _lib


def layer_shape(width, height, slices):
    return (slices, (height + 3) // 4, (width + 3) // 4) if slices == 16 else (1, height, width)


def scissor(guard_band, slices):
    return guard_band // int(np.sqrt(float(slices)) + 0.5) if slices > 1 else guard_band


def inside(width, height, slices, guard_band):
    """Boolean mask [slices][qh][qw] of the texels inside the scissor."""
    S, qh, qw = layer_shape(width, height, slices)
    g = scissor(guard_band, slices)
    m = np.zeros((S, qh, qw), bool)
    if 2 * g < qw and 2 * g < qh:
        m[:, g:qh - g, g:qw - g] = True
    return m


def make_net(name, slices, seed=0):
    """Seeded random layers [(weights [S][K][K][Cin][Cout], bias [S][Cout])] of net `name`, distinct per slice.
    The weights are drawn symmetric around zero with a spread of scale / sqrt(fan-in) x 2.5 and the biases around a
    small positive value, so that pre-activations of both signs occur, ReLU clips some and passes others, and the last
    layer lands below dark, above bright and in between (asserted on the checker's counters in test_convnet.py)."""
    k, ch = NETS[name]
    scale = NET_SCALE.get(name, 1.0)
    rng = np.random.default_rng([ord(name), slices, seed])
    layers = []
    for cin, cout in zip(ch[:-1], ch[1:]):
        w = rng.normal(0.0, 2.5 * scale / np.sqrt(cin * k * k), (slices, k, k, cin, cout)).astype(F)
        b = rng.normal(0.05, 0.1, (slices, cout)).astype(F)
        layers.append((w, b))
    # the last layer: centred on the AO range so that the clamp sees all three cases
    w, b = layers[-1]
    b[:, 0] = rng.uniform(0.3, 0.6, slices).astype(F)
    return layers


def synthetic(width, height, slices):
    """One synthetic input set as layers: R8 bright in [60, 255] and dark a random share of it (dark <= bright), except
    a 3 x 2 patch per slice where dark > bright; R8 importance; float depth, a ramp in [0, 1) with noise (what
    scripts/SAVO_record.py feeds: linear depth / 1000 -- scaled up here so that the channel matters).  Read-only."""
    S, qh, qw = layer_shape(width, height, slices)
    rng = np.random.default_rng([width, height, slices])
    bright = rng.integers(60, 256, (S, qh, qw)).astype(np.uint8)
    dark = (bright * rng.uniform(0.1, 0.95, (S, qh, qw))).astype(np.uint8)
    y0, x0 = qh // 2, qw // 2
    dark[:, y0:y0 + 2, x0:x0 + 3] = 250
    bright[:, y0:y0 + 2, x0:x0 + 3] = 90
    importance = rng.integers(0, 256, (S, qh, qw)).astype(np.uint8)
    yy, xx = np.mgrid[0:qh, 0:qw]
    depth = ((0.1 + 0.8 * (xx + 2 * yy) / (qw + 2 * qh))[None] * rng.uniform(0.8, 1.2, (S, qh, qw))).astype(F)
    out = dict(bright=bright, dark=dark, importance=importance, depth=depth)
    for a in out.values():
        a.setflags(write=False)
    return out


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def run(lib, layers, inputs, width, height, guard_band=0, precision=FLOAT, clamp_output=True, fill=SENTINEL):
    """The checker on `layers` ([(weights, bias or None)]) and `inputs` (a list of up to four [S][qh][qw] uint8 or
    float32 arrays: bright, dark, importance, depth).  Returns dict(out [S][qh][qw] float32 -- texels outside the
    scissor keep `fill` --, inter: the stored activations of every layer but the last as float32 [S][Cout][qh][qw], 0
    outside the scissor, bound [S][qh][qw] float64, counters)."""
    L = len(layers)
    ws = [np.ascontiguousarray(w, F) for w, _ in layers]
    bs = [None if b is None else np.ascontiguousarray(b, F) for _, b in layers]
    S = ws[0].shape[0]
    ins = [np.ascontiguousarray(a) for a in inputs]
    assert all(a.dtype in (np.uint8, np.float32) and a.shape == layer_shape(width, height, S) for a in ins)
    assert len(ins) >= ws[0].shape[3] and (not clamp_output or len(ins) >= 2)
    _, qh, qw = ins[0].shape
    K = (C.c_int * L)(*[w.shape[1] for w in ws])
    Cin = (C.c_int * L)(*[w.shape[3] for w in ws])
    Cout = (C.c_int * L)(*[w.shape[4] for w in ws])
    for l, w in enumerate(ws):
        assert w.shape[1] == w.shape[2] and w.shape[0] == S and (l == 0 or w.shape[3] == ws[l - 1].shape[4])
    wp = (C.c_void_p * L)(*[w.ctypes.data for w in ws])
    bp = (C.c_void_p * L)(*[None if b is None else b.ctypes.data for b in bs])
    ip = (C.c_void_p * 4)(*[ins[c].ctypes.data if c < len(ins) else None for c in range(4)])
    ib = (C.c_int * 4)(*[ins[c].itemsize if c < len(ins) else 4 for c in range(4)])
    out = np.full((S, qh, qw), fill, F)
    inter = [np.zeros((S, w.shape[4], qh, qw), F) for w in ws[:-1]]
    tp = (C.c_void_p * max(L - 1, 1))(*([a.ctypes.data for a in inter] or [None]))
    bound = np.zeros((S, qh, qw), np.float64)
    counters = np.zeros(len(COUNTERS), np.uint64)
    lib.convnet_ref(L, S, K, Cin, Cout, wp, bp, qw, qh, scissor(guard_band, S), ip, ib, int(precision), int(bool(clamp_output)),
                    _p(out), tp, _p(bound), _p(counters))
    return dict(out=out, inter=inter, bound=bound, counters=dict(zip(COUNTERS, (int(v) for v in counters))))


def input_list(syn, cin0=4):
    """The inputs a net of cin0 first-layer channels needs (at least bright and dark, for the clamp)."""
    return [syn[k] for k in ("bright", "dark", "importance", "depth")][:max(cin0, 2)]
