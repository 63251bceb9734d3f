"""librsd's texture sampler rule on the host (csrc/tex_sample.h): 8 sub-texel bits with a carry into the next texel,
wrap / clamp addressing, the x-then-y lerp, the clamp point sampler and the guard-band uv bounds -- the one definition
every kernel that filters a texture calls.

tests/native/check_tex_sample.cpp evaluates the header over a fixed case list under AddressSanitizer and UBSan
(float-cast-overflow included: tex_point converts no out-of-range float) and prints inputs and results; here every
line is recomputed with a float32 numpy restatement, independent of oracle/, and compared exactly.  The cases, on axes
of 1, 2, 3 and 5 texels: pixel centres, the carry (a fraction of 255.9 / 256), the last fraction below it (255.4 / 256),
a fraction with a non-zero weight, all of these left of texel 0 (ix = -1, ix = -n - 1) and right of texel n - 1
(ix + 1 == n and beyond), u = 0 and u = 1 exactly; tex_point at 0, just below 1, 1, negative, 2, huge, infinite, NaN."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
CSRC = HERE.parent / "ray-traced-stochastic-depth-map_amd" / "csrc"
F = np.float32
TEXELS = [F(0.125), F(0.7), F(1.0) / F(3.0), F(0.9)]  # t00, t10, t01, t11 of the program's lerp


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("tex_sample") / "check_tex_sample"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
                    "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", f"-I{CSRC}", "-o", str(exe), str(HERE / "native" / "check_tex_sample.cpp")],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    rows = {}
    for ln in out.stdout.splitlines():
        f = ln.replace("|", " ").split()
        rows.setdefault(f[0], []).append(f[1:])
    return rows


def _f32(col):
    return np.array([int(v, 16) for v in col], np.uint32).view(np.float32)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _axis(u, n):
    """The rule on one axis, float32 operation by operation: index before addressing, q in 256ths, weight"""
    x = u * n.astype(F) - F(0.5)
    f0 = np.floor(x)
    q = np.floor((x - f0) * F(256.0) + F(0.5))
    carry = q >= F(256.0)
    i = f0.astype(np.int64) + carry
    q = np.where(carry, F(0.0), q).astype(F)
    return i, q, q * (F(1.0) / F(256.0))


def _addr(i, n, wrap):
    return np.where(wrap, np.mod(i, n), np.clip(i, 0, n - 1))  # numpy's mod takes the divisor's sign: non-negative


def test_split_taps_and_lerp(lines):
    S = np.array(lines["S"])
    W, H, kx, fx, ky, fy = (S[:, c].astype(np.int64) for c in range(6))
    u, v = _f32(S[:, 6]), _f32(S[:, 7])
    got_i = S[:, 8:10].astype(np.int64)
    got_q = np.stack([_f32(S[:, 10]), _f32(S[:, 11])], 1)
    got_w = np.stack([_f32(S[:, 12]), _f32(S[:, 13])], 1)
    ix, qx, wx = _axis(u, W)
    iy, qy, wy = _axis(v, H)
    assert np.array_equal(got_i, np.stack([ix, iy], 1))
    assert np.array_equal(_bits(got_q), _bits(np.stack([qx, qy], 1)))
    assert np.array_equal(_bits(got_w), _bits(np.stack([wx, wy], 1)))
    # what each kind of case is there for, stated without the rule: (index - k, q)
    want = {0: (0, 0.0), 1: (0, 77.0), 2: (0, 255.0), 3: (1, 0.0), 4: (0, 128.0), 5: (0, 128.0)}
    for c, k, kind, i, q, n in ((u, kx, fx, ix, qx, W), (v, ky, fy, iy, qy, H)):
        for code, (di, qq) in want.items():
            m = kind == code
            assert m.any() and np.array_equal(i[m], k[m] + di) and np.all(q[m] == qq), code
        assert (i == -1).any() and (i == -n - 1).any() and (i + 1 == n).any() and (i > n).any()
        assert np.all(c[kind == 4] == 0.0) and np.all(c[kind == 5] == 1.0)
    # addressed taps, wrap then clamp: t00 t10 t01 t11 as offsets y * W + x
    for c0, wrap in ((14, True), (18, False)):
        x0, x1, y0, y1 = _addr(ix, W, wrap), _addr(ix + 1, W, wrap), _addr(iy, H, wrap), _addr(iy + 1, H, wrap)
        assert np.array_equal(S[:, c0:c0 + 4].astype(np.int64), np.stack([y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1], 1))
        one = (W == 1) & (H == 1)
        assert one.any() and np.all(S[one, c0:c0 + 4].astype(np.int64) == 0), "a 1 x 1 texture: every tap is texel 0"
    # the lerp: x pairs first, then y, each operation rounded
    t00, t10, t01, t11 = TEXELS
    r0 = t00 * (F(1.0) - wx) + t10 * wx
    r1 = t01 * (F(1.0) - wx) + t11 * wx
    assert np.array_equal(_bits(_f32(S[:, 22])), _bits(r0 * (F(1.0) - wy) + r1 * wy))
    assert ((wx != 0) & (wy != 0)).any()


def test_addr(lines):
    A = np.array(lines["A"]).astype(np.int64)
    i, n, wrap, got = A.T
    assert np.array_equal(got, _addr(i, n, wrap != 0))
    assert np.all((got >= 0) & (got < n)) and (i < -n).any() and (i > n).any()


def test_point(lines):
    P = np.array(lines["P"])
    uv, n, got = _f32(P[:, 0]), P[:, 1].astype(np.int64), P[:, 2].astype(np.int64)
    with np.errstate(invalid="ignore"):
        f = np.floor(uv * n.astype(F))
    want = np.clip(np.nan_to_num(f, nan=0.0, posinf=1e9, neginf=-1e9), 0, n - 1).astype(np.int64)  # clamped as a float
    assert np.array_equal(got, want)
    below1 = uv == np.nextafter(F(1.0), F(0.0))
    assert np.all(got[np.isnan(uv)] == 0) and np.all(got[uv <= 0] == 0) and below1.any()
    assert np.all(got[(uv >= 1.0) | below1] == n[(uv >= 1.0) | below1] - 1)
    assert np.isnan(uv).any() and np.isinf(uv).any() and (np.abs(uv) > 2.0 ** 31).any()


def test_guard_uv(lines):
    G = np.array(lines["G"])
    W, H, g = (G[:, c].astype(np.int64).astype(F) for c in range(3))
    want = [(g + F(0.5)) / W, (g + F(0.5)) / H, (W - (g + F(0.5))) / W, (H - (g + F(0.5))) / H]  # GuardBand.cpp:62-63
    for c, w in enumerate(want):
        assert np.array_equal(_bits(_f32(G[:, 3 + c])), _bits(w))
