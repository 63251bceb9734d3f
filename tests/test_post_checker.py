"""CPU checks of the post-AO passes' checker (tests/native/post_ref.c, tests/post_checker.py): known answers that pin
it to the shader text, its agreement with oracle/ on the inputs of the older GPU tests, and the input conditions of
tests/test_gpu_post_edges.py, shown on the checker alone (the thresholds below are conditions, not measurements)."""
import ctypes as C
import math

import numpy as np
import pytest

import post_checker as PC
from helpers import to_oracle

F = np.float32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return PC.build(tmp_path_factory.mktemp("post_ref"))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ texture rules

def test_store_and_min_max_rules(lib):
    """UNORM8 store: NaN -> 0, clamped, round half up (0.5 / 255 steps); HLSL min / max return the non-NaN operand."""
    assert lib.post_store_unorm8(float("nan")) == 0 and lib.post_store_unorm8(-3.0) == 0
    assert lib.post_store_unorm8(7.0) == 255 and lib.post_store_unorm8(float("inf")) == 255
    assert lib.post_store_unorm8(0.5) == 128                      # 127.5 + 0.5 -> 128: half up
    assert lib.post_store_unorm8(float(F(1.5) / F(255))) == 2     # 1.5 -> 2, where half-to-even agrees
    assert lib.post_store_unorm8(float(F(2.5) / F(255))) == 3     # 2.5 -> 3, where half-to-even would give 2
    nan = float("nan")
    assert lib.post_hlsl_min(nan, 2.0) == 2.0 and lib.post_hlsl_min(2.0, nan) == 2.0
    assert lib.post_hlsl_max(nan, -2.0) == -2.0 and lib.post_hlsl_max(-2.0, nan) == -2.0
    assert math.isnan(lib.post_hlsl_min(nan, nan))


def test_linear_sampling_rule(lib):
    """8-bit sub-texel weights: a fraction of k/256 + 1/512 rounds up to (k + 1)/256, a fraction that rounds to 256
    moves to the next texel; clamp addressing at both ends."""
    i0, w = C.c_int(), C.c_float()
    for p, want_i, want_w in ((3.0, 3, 0.0), (3.0 + 7 / 256 + 1 / 512, 3, 8 / 256), (3.0 + 7 / 256 + 0.9 / 512, 3, 7 / 256),
                              (3.0 + 255 / 256 + 1 / 512, 4, 0.0), (-0.25, -1, 0.75)):
        lib.post_linear_axis(float(F((p + 0.5) / 8)), 8, C.byref(i0), C.byref(w))   # 8 texels: uv * 8 is exact
        assert (i0.value, w.value) == (want_i, want_w), p
    t = np.array([[10, 250]], np.uint8)
    assert lib.post_sample_unorm8_clamp(t.ctypes.data_as(C.c_void_p), 2, 1, 0.5, 0.5) == \
        float(F(10) / F(255) * F(0.5) + F(250) / F(255) * F(0.5))
    assert lib.post_sample_unorm8_clamp(t.ctypes.data_as(C.c_void_p), 2, 1, -3.0, 9.0) == float(F(10) / F(255))


# ------------------------------------------------------------------------------------------------ blur

def test_blur_constant_image_stays_constant(lib):
    c = PC.blur_case(65, 9)
    for R in (1, 4, 20):
        out, _ = PC.blur(lib, np.full((9, 65), 77, np.uint8), np.abs(np.nan_to_num(c["z"], posinf=9.0)) + 1, 0, R, True)
        assert (out == 77).all(), R


@pytest.mark.parametrize("R", [1, 4, 20])
def test_blur_weights_known_answers(lib, R):
    """Equal depths: w(d) = exp2(-d^2 / (2 sigma^2)), sigma = (R + 1) / 2, in Python double (the float32 argument
    -d^2 * falloff carries two roundings: 4 ulp of slack).  A perfect ramp: betterSlope removes the slope at every
    tap; the other slope (taken at the first tap of each side) does so too on a ramp, and on a bent ramp only its
    first tap keeps the pure falloff weight."""
    sigma = (R + 1) / 2
    want = np.array([2.0 ** (-(d * d) / (2 * sigma * sigma)) for d in range(-R, R + 1)])
    flat = PC.blur_weights(lib, np.full(2 * R + 1, 3.0, F), True)
    assert np.abs(flat - want).max() <= 4 * np.spacing(F(1.0))
    ramp = (8.0 + 0.25 * np.arange(-R, R + 1)).astype(F)   # multiples of 0.25: every difference is exact
    for better in (True, False):
        assert np.array_equal(_bits(PC.blur_weights(lib, ramp, better)), _bits(flat)), better
    if R >= 4:
        bent = ramp.copy()
        bent[R + 2:] += F(0.5)
        bent[:R - 1] -= F(0.25)
        w = PC.blur_weights(lib, bent, False)
        assert w[R + 1] == flat[R + 1] and w[R - 1] == flat[R - 1]
        assert w[R + 2] < flat[R + 2] and w[R - 2] < flat[R - 2]
        # the second side runs with the slope negated: a ramp that is flat on the left of the centre
        kink = np.where(np.arange(-R, R + 1) <= 0, F(8.0), ramp).astype(F)
        w = PC.blur_weights(lib, kink, True)     # min slope 0: the left side keeps the falloff, the right side does not
        assert np.array_equal(_bits(w[:R]), _bits(flat[:R])) and (w[R + 1:] < flat[R + 1:]).all()


# ------------------------------------------------------------------------------------------------ TAA

def test_taa_static_history_is_a_lerp(lib):
    """Zero motion, a constant history and a box wide enough (sigma 50 on a noisy colour): lerp(hist, color, alpha)."""
    rng = np.random.default_rng(3)
    H, W = 7, 9
    color = (rng.random((H, W, 4)) * 2).astype(F)
    hist = np.full((H, W, 4), F(0.75))
    out = PC.taa(lib, color, np.zeros((H, W, 2), F), hist, alpha=0.25, sigma=50.0, anti_flicker=False)
    want = 0.75 + 0.25 * (color[..., :3].astype(np.float64) - 0.75)
    assert np.abs(out[..., :3] - want).max() < 1e-6 and (out[..., 3] == 1).all()


def test_catmull_rom_weights_sum_to_one(lib):
    """The nine weights the shader applies, the products of (w0, w12, w3) in x and in y (TAA.ps.slang:64-73),
    summed in float32 in the shader's order, are 1 to 4 ulp at 50 random fractions."""
    rng = np.random.default_rng(4)
    for fx, fy in rng.random((50, 2)):
        wx, tcx = PC.catmull_rom_axis(lib, 10.5 + fx, 32.0)
        wy, _ = PC.catmull_rom_axis(lib, 3.5 + fy, 16.0)
        ax, ay = [wx[0], wx[1] + wx[2], wx[3]], [wy[0], wy[1] + wy[2], wy[3]]
        total = F(0)
        for i in range(3):
            for j in range(3):
                total = F(total + F(ax[i] * ay[j]))
        assert abs(float(total) - 1.0) <= 4 * np.spacing(F(1.0)), (fx, fy, total)
        assert tcx[0] == F(9.5) / F(32) and tcx[2] == F(12.5) / F(32)
    w, tc = PC.catmull_rom_axis(lib, 10.5, 32.0)   # on a texel centre: all the weight on the centre tap
    assert list(w) == [0.0, 1.0, 0.0, 0.0] and tc[1] == F(10.5) / F(32)


# ------------------------------------------------------------------------------------------------ dilation

def test_dilation_ring_of_one_texel(lib):
    """The five Gathers sample at the pixel centre and at (+0.5, +1.5), (+1.5, -0.5), (-0.5, -1.5), (-1.5, +0.5) px
    from it; a sample at (a, b) px from a centre has the footprint {floor(a), floor(a) + 1} x {floor(b), floor(b) +
    1} (fractions of exactly one half: weight 128 / 256, no tie).  So pixel p reads p + the 17 distinct offsets below (the five footprints overlap in three texels), and a
    single set texel s lights, under max, exactly s minus them."""
    pts = [(0.0, 0.0), (0.5, 1.5), (1.5, -0.5), (-0.5, -1.5), (-1.5, 0.5)]
    reads = {(math.floor(a) + i, math.floor(b) + j) for a, b in pts for i in (0, 1) for j in (0, 1)}
    # the centre Gather at an exact texel centre has fraction 0: its footprint is the texel and its +1 neighbours
    assert len(reads) == 17 and {(0, 0), (1, 1), (0, 2), (2, -1), (-1, -2), (-2, 1)} <= reads
    H, W, sy, sx = 16, 16, 8, 7
    m = np.zeros((H, W), np.uint8)
    m[sy, sx] = 1
    want = np.zeros_like(m)
    for dx, dy in reads:
        want[sy - dy, sx - dx] = 1
    assert np.array_equal(PC.binary_dilation(lib, m, True), want)
    assert np.array_equal(PC.binary_dilation(lib, 1 - m, False), 1 - want)


# ------------------------------------------------------------------------------------------------ TemporalAO

def test_temporal_history_saturates_and_does_not_wrap(lib):
    cam, _ = PC.cameras(8, 4)
    H, W = 4, 8
    z = np.full((H, W), 5.0, F)
    ident = np.eye(4, dtype=F)
    for n_in, n_out in ((0, 1), (1, 2), (28, 29), (29, 30), (30, 30), (200, 30), (255, 30)):
        ao, n, fl, _ = PC.temporal_ao(lib, np.full((H, W), 255, np.uint8), z, np.zeros((H, W, 2), F), z,
                                      np.zeros((H, W), np.uint8), np.full((H, W), n_in, np.uint8), None, 0, cam, ident)
        assert (n == n_out).all() and (fl == PC.ACCUMULATED).all()
        want = int(np.floor(F(1) / F(n_in + 1) * F(255) + F(0.5)))   # (prevN * 0 + 1) / (prevN + 1); 255 + 1 = 256, no wrap to 0
        assert (ao == want).all() and want >= 1, n_in


# ------------------------------------------------------------------------------------------------ de/interleave

def test_deinterleave_round_trip_every_residue(lib):
    rng = np.random.default_rng(5)
    for W in range(5, 9):
        for H in range(5, 9):
            a = rng.integers(1, 256, (H, W, 2)).astype(np.uint8)
            layers = PC.deinterleave(lib, a)
            assert layers.shape == (16, 2, 2, 2)
            assert np.array_equal(layers[6, 1, 0], a[5, 2] if H > 5 else [0, 0])   # layer 6 = offset (2, 1): src[4 + 1][0 + 2]
            assert np.array_equal(PC.interleave(lib, layers, W, H), a), (W, H)


def test_ray_min_max_length_known(lib):
    mn, mx = np.array([1.0, 5.0, 3.0], F).view(np.uint32), np.array([33.0, 2.0, 0.0], F).view(np.uint32)
    assert list(PC.ray_min_max_length(lib, mn, mx)) == [1.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------------ motion vectors

MV_EXCLUDE, MV_EXCLUDED_SHARE = 0.05, 0.02
MV_BOUND = 4 * 2.25e-7


def test_motion_vectors_against_double(lib):
    """The checker's float32 motion vectors against the same projection in Python double, over the four poses at
    129 x 9 and 65 x 5 and depths 2 .. 30.  Worst |difference| seen: 2.25e-7 (uv units); bound 4 x that = 9e-7,
    the double reference orders its operations differently.  Points with pw < 5 % of |rel| (pw along the previous camera's unit view axis) are excluded (at most
    2 % of the geometry pixels of a pose); the pose "behind" is all (2, 2) and is checked as such."""
    worst = 0.0
    for W, H in ((129, 9), (65, 5)):
        cur, prevs = PC.cameras(W, H)
        rng = np.random.default_rng(W)
        z = (2.0 + 28.0 * rng.random((H, W))).astype(F)
        z[0, :7] = cur.farZ
        for name, prev in prevs.items():
            got, ratio = PC.motion_vectors(lib, cur, prev, z)
            geo = z < F(cur.farZ)
            assert (got[~geo] == 0).all()
            if name == "behind":
                assert (got[geo] == 2).all()
                continue
            keep = geo & (ratio >= MV_EXCLUDE)
            assert (geo & ~keep).sum() <= MV_EXCLUDED_SHARE * geo.sum(), name
            want = PC.motion_vectors_double(cur, prev, z)
            err = float(np.abs(got[keep].astype(np.float64) - want[keep]).max())
            worst = max(worst, err)
            assert np.abs(got[keep]).max() > 0.01, name   # the pose moves the image
    print(f"motion vectors: worst |float32 - double| = {worst:.3g}, bound {MV_BOUND:.3g}")
    assert worst <= MV_BOUND


# ------------------------------------------------------------------------------------------------ the oracle

def test_agrees_with_oracle_on_the_older_tests_inputs(lib, oracle):
    """Checker and oracle bit for bit on the inputs of tests/test_gpu_post.py and tests/test_gpu_temporal.py."""
    from oracle.texops import deinterleave, interleave, ray_min_max_length
    from rsd.frame import FrameConfig, look_at
    from rsd.temporal import prev_view_to_cur_view
    for radius, better, guard in [(4, 1, 16), (1, 1, 0), (7, 0, 8), (20, 1, 3)]:
        rng = np.random.default_rng(radius)
        H, W = 67, 131
        yy, xx = np.mgrid[0:H, 0:W]
        z = (5.0 + 3.0 * np.sin(xx / 9.0) + (xx > 70) * 20.0 + 0.01 * yy).astype(F)
        src = rng.integers(0, 256, (H, W)).astype(np.uint8)
        want, want_pp = oracle.cross_bilateral_blur(src, z, guard, radius, bool(better), dst=np.full((H, W), 9, np.uint8))
        got, got_pp = PC.blur(lib, src, z, guard, radius, better, fill=9)
        assert np.array_equal(got, want), radius
        s = slice(guard, H - guard), slice(guard, W - guard)
        assert np.array_equal(got_pp[s], want_pp[s]), radius
    for guard, use_mask in [(0, False), (16, True), (5, False)]:
        rng = np.random.default_rng(guard)
        H, W = 90, 150
        cfg = FrameConfig(visible_w=W, visible_h=H, guard_band=0)
        c0 = look_at([0.0, 2.0, 8.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0], cfg)
        c1 = look_at([0.2, 2.1, 7.7], [0.1, 1.0, 0.0], [0.0, 1.0, 0.0], cfg)
        m = np.ascontiguousarray(prev_view_to_cur_view(c1, c0), F)
        ao = rng.integers(0, 256, (H, W)).astype(np.uint8)
        z = (2.0 + 10.0 * rng.random((H, W))).astype(F)
        mv = (rng.normal(0.0, 0.01, (H, W, 2))).astype(F)
        mv[rng.random((H, W)) < 0.1] = 0.7
        mv[rng.random((H, W)) < 0.1] = 0.0
        prev_z = (z * (1.0 + rng.uniform(-0.2, 0.2, (H, W)))).astype(F)
        prev_z[rng.random((H, W)) < 0.02] = 0.0
        prev_ao = rng.integers(0, 256, (H, W)).astype(np.uint8)
        prev_n = rng.integers(0, 31, (H, W)).astype(np.uint8)
        mask = (rng.random((H, W)) < 0.2).astype(np.uint8) if use_mask else None
        want, want_n = oracle.temporal_ao(ao, z, mv, prev_z, prev_ao, prev_n, to_oracle(c1, oracle.Camera), m, guard,
                                          stable_mask=mask, ao_dst=np.full((H, W), 7, np.uint8),
                                          history_dst=np.full((H, W), 7, np.uint8))
        got, got_n, _, _ = PC.temporal_ao(lib, ao, z, mv, prev_z, prev_ao, prev_n, mask, guard, c1, m, fill=7)
        assert np.array_equal(got, want) and np.array_equal(got_n, want_n), guard
    # motion vectors, both entries
    cfg = FrameConfig(visible_w=160, visible_h=96, guard_band=16)
    c0 = look_at((0.0, 2.0, 8.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), cfg)
    c1 = look_at((0.6, 2.2, 7.5), (0.1, 1.0, 0.0), (0.0, 1.0, 0.0), cfg)
    rng = np.random.default_rng(11)
    z = (4.0 + 20.0 * rng.random((cfg.fb_h, cfg.fb_w))).astype(F)
    z[: cfg.fb_h // 3] = c1.farZ
    oc1, oc0 = to_oracle(c1, oracle.Camera), to_oracle(c0, oracle.Camera)
    assert np.array_equal(_bits(PC.motion_vectors(lib, c1, c0, z)[0]), _bits(oracle.motion_vectors(oc1, oc0, z)))
    d = np.random.default_rng(12).uniform(0.5, 0.99, (cfg.fb_h, cfg.fb_w)).astype(F)
    d[: cfg.fb_h // 3] = 1.0
    assert np.array_equal(_bits(PC.motion_vectors(lib, c1, c0, d, raw=True)[0]),
                          _bits(oracle.motion_vectors_raster(oc1, oc0, d)))
    # TAA
    for sigma, anti in [(1.0, True), (0.5, False), (4.0, True)]:
        rng = np.random.default_rng(int(sigma * 10))
        H, W = 45, 77
        frames = [(rng.random((H, W, 4)) * 2).astype(F) for _ in range(3)]
        mvs = [rng.normal(0.0, 0.02, (H, W, 2)).astype(F) for _ in range(3)]
        mvs[1][:5] = 0.6
        prev = np.zeros((H, W, 4), F)
        for c, mv in zip(frames, mvs):
            want = oracle.taa(c, mv, prev, alpha=0.1, color_box_sigma=sigma, anti_flicker=anti)
            assert np.array_equal(_bits(PC.taa(lib, c, mv, prev, 0.1, sigma, anti)), _bits(want)), sigma
            prev = want
    # flicker mask and dilation
    rng = np.random.default_rng(11)
    H, W = 70, 110
    cam = look_at([0.3, 2.0, 8.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0], FrameConfig(visible_w=W, visible_h=H, guard_band=0))
    z = (4.0 + np.cumsum(rng.normal(0, 0.05, (H, W)), axis=1)).astype(F)
    z[:, 40:] += 3.0
    z[5:9, 5:9] = z[5:9, 5:9][::-1]
    n = rng.normal(0, 1, (H, W, 4)).astype(F)
    n[..., :3] /= np.linalg.norm(n[..., :3], axis=-1, keepdims=True)
    n[::3, ::3, :3] = [0.0, 0.0, 1.0]
    want = oracle.ao_flicker_mask(z, n, to_oracle(cam, oracle.Camera))
    assert np.array_equal(PC.flicker_mask(lib, z, n, cam)[0], want)
    for op in (0, 1):
        assert np.array_equal(PC.binary_dilation(lib, want, op), oracle.binary_dilation(want, "max" if op else "min"))
    # deinterleave / interleave, ray lengths
    for shape, dtype in [((37, 70), np.float32), ((64, 40, 4), np.float32), ((21, 33), np.uint8), ((18, 18, 2), np.float32)]:
        a = (np.random.default_rng(sum(shape)).random(shape) * 255).astype(dtype)
        want = deinterleave(a)
        assert np.array_equal(PC.deinterleave(lib, a), want)
        assert np.array_equal(PC.interleave(lib, want, shape[1], shape[0]), interleave(want, shape[0], shape[1]))
    rng = np.random.default_rng(5)
    mn = (rng.random((45, 77)) * 50).astype(F)
    mx = (mn + (rng.random((45, 77)) * 10 - 2)).astype(F)
    mxu = mx.view(np.uint32).copy()
    mxu[rng.random((45, 77)) < 0.2] = 0
    assert np.array_equal(_bits(PC.ray_min_max_length(lib, mn.view(np.uint32), mxu)),
                          _bits(ray_min_max_length(mn.view(np.uint32), mxu)))


def test_image_equation_agrees_with_oracle(lib):
    """The evaluator of post_checker.py against oracle/image_eq.py on the older test's formulas and inputs."""
    from oracle import image_eq as IE
    from test_gpu_post import FORMULAS
    rng = np.random.default_rng(2)
    H, W = 37, 70
    imgs = [rng.integers(0, 256, (H, W)).astype(np.uint8), (rng.random((H, W, 4)) * 3 - 1).astype(F),
            rng.random((H - 5, W - 9, 2)).astype(F), (rng.random((H, W)) * 4 - 2).astype(F)]
    fmts = [IE.FMT_R8UNORM, IE.FMT_RGBA32F, IE.FMT_RG32F, IE.FMT_R32F]
    for formula in FORMULAS:
        want = IE.evaluate(formula, list(zip(imgs, fmts)), W, H)
        (_, got, _), fragile = PC.image_equation(formula, list(zip(imgs, fmts)), W, H)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), formula
        assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), formula
        assert np.array_equal(PC.store(lib, got, PC.R8UNORM), IE.store(want, IE.FMT_R8UNORM)), formula


# ------------------------------------------------------------------------------------------------ input conditions

def test_image_equation_cases(lib):
    """Every formula of the GPU module compiles in librsd with the stack it is meant to need (the depth-9 one is
    refused), the info call reports the inputs it reads, at most 1 texel in 1000 is fragile, and the formulas as
    folded into [0, 1) for the R8Unorm target store a byte strictly between 0 and 255 on at least 90 % of the texels."""
    from rsd import abi
    open_bytes = total_bytes = 0
    for W, H in PC.SIZES:
        inputs = PC.image_inputs(W, H)
        for formula, names in [e for e in PC.EQUATIONS] + [(PC.unorm_formula(f), n) for f, n in PC.EQUATIONS]:
            h = C.c_void_p()
            assert abi.lib().rsd_image_equation_compile(formula.encode(), C.byref(h)) == abi.RSD_OK, formula
            n, mask = C.c_uint32(), C.c_uint32()
            assert abi.lib().rsd_image_equation_info(h, C.byref(n), C.byref(mask)) == abi.RSD_OK
            abi.lib().rsd_image_equation_release(h)
            assert mask.value == sum(1 << k for k, name in enumerate(names) if name) and 1 <= n.value <= 64
            (lo, mid, hi), fragile = PC.image_equation(formula, [inputs[k] if k else (None, 0) for k in names], W, H)
            assert np.isfinite(mid).all(), formula
            if formula.startswith("frac(("):   # the R8Unorm run: the stored byte must not be pinned at 0 or 255
                b = PC.store(lib, mid, PC.R8UNORM)
                open_bytes, total_bytes = open_bytes + int(((b > 0) & (b < 255)).sum()), total_bytes + b.size
            assert fragile.sum() * 1000 <= fragile.size, (formula, int(fragile.sum()))
            assert np.array_equal(_bits(lo)[~fragile], _bits(mid)[~fragile]) and \
                np.array_equal(_bits(hi)[~fragile], _bits(mid)[~fragile]), formula
    print("R8Unorm stores strictly between 0 and 255:", open_bytes, "of", total_bytes)
    assert open_bytes >= 0.9 * total_bytes
    h = C.c_void_p()
    assert abi.lib().rsd_image_equation_compile(PC.DEPTH9.encode(), C.byref(h)) != abi.RSD_OK and not h.value
    assert "nested too deeply" in abi.lib().rsd_last_error().decode()
    # one value fewer on the stack compiles, so DEPTH8 sits exactly on the limit
    assert PC.DEPTH9.replace("0.5 * (", "", 1)[:-1] == PC.DEPTH8


def _tao_cases(lib):
    cam, _ = PC.cameras(129, 9)
    for (W, H) in PC.SIZES + [(67, 19)]:
        for guard in (0, 5):
            if 2 * guard >= min(W, H):
                continue
            for use_mask in (False, True):
                yield PC.tao_case(lib, W, H, guard, use_mask, cam), (W, H, guard, use_mask), cam


def test_temporal_ao_cases_reach_their_branches(lib):
    """Over the TemporalAO cases of the GPU module, on the checker alone: at least 50 texels exactly on each limit
    of the valid area, one float inside and one float outside it, each taking the intended side; at least 50 with
    the depth test value within 2^-23 below 0.1 and 50 within 2^-23 at or above it (the quotient near 0.9 moves in
    steps of 2^-24, so one float32 step of 0.1 is not reachable); 50 on bilinear ties and 50 on texel centres; both
    branches at least 10 % of every scissor of 40 texels or more."""
    count = {}
    for c, (W, H, guard, use_mask), cam in _tao_cases(lib):
        ao, n, fl, pd = PC.temporal_ao(lib, c["ao"], c["z"], c["mv"], c["prev_z"], c["prev_ao"], c["prev_n"], c["mask"],
                                       guard, cam, c["m"])
        cat = c["cat"]
        s = slice(guard, H - guard), slice(guard, W - guard)
        assert (ao[:guard] == PC.SENTINEL).all() and (n[:, :guard] == PC.SENTINEL).all()
        inside = {"minx_below": False, "minx_on": True, "minx_above": True, "maxx_below": True, "maxx_on": True,
                  "maxx_above": False, "miny_below": False, "miny_on": True, "miny_above": True, "maxy_below": True,
                  "maxy_on": True, "maxy_above": False}
        for name, want_in in inside.items():
            sel = cat[name]
            assert (((fl[sel] & PC.OUTSIDE) == 0) == want_in).all(), (name, W, H, guard)
            if want_in:
                assert (fl[sel] == PC.ACCUMULATED).all(), name
                sel = sel & (n != 1)   # counted where the side shows in the output: history > 1 inside, 1 outside
            count[name] = count.get(name, 0) + int(sel.sum())
        assert (fl[cat["ratio_in"]] == PC.ACCUMULATED).all() and (fl[cat["ratio_out"]] == PC.DEPTH_REJECT).all()
        assert (fl[cat["depth0"]] == PC.DEPTH_REJECT).all()
        for name, want_n in (("n0", 1), ("n29", 30), ("n30", 30), ("n255", 30)):
            assert (n[cat[name]] == want_n).all() and (fl[cat[name]] == PC.ACCUMULATED).all(), name
        i0, w = C.c_int(), C.c_float()
        for name in ("tie", "centre"):
            for y, x in zip(*np.nonzero(cat[name])):
                assert fl[y, x] == PC.ACCUMULATED
                for uv, size in ((c["tu"][y, x] + c["mv"][y, x, 0], W), (c["tv"][y, x] + c["mv"][y, x, 1], H)):
                    p = F(F(uv) * F(size)) - F(0.5)
                    frac = float(p - np.floor(p)) * 256
                    assert (frac - math.floor(frac) == 0.5) if name == "tie" else (frac == 0), (name, x, y)
        for name in ("ratio_in", "ratio_out", "depth0", "prev_depth0", "n0", "n29", "n30", "n255", "tie", "centre"):
            count[name] = count.get(name, 0) + int(cat[name].sum())
        if fl[s].size >= 40:
            acc, reset = (fl[s] == PC.ACCUMULATED).mean(), (fl[s] != PC.ACCUMULATED).mean()
            assert acc >= 0.1 and reset >= 0.1, (W, H, guard, acc, reset)
        if use_mask and fl[s].size >= 40:
            assert (fl[s] & PC.STABLE).any()
    print("TemporalAO texels per category:", count)
    assert all(v >= 50 for k, v in count.items() if k not in ("depth0", "prev_depth0")), count
    assert count["depth0"] >= 50 and count["prev_depth0"] >= 50


def test_taa_cases_reach_their_paths(lib):
    """The TAA cases, classified by the motion each texel samples with (the longest of its 3 x 3 neighbourhood,
    TAA.ps.slang:121-127, restated in post_checker.taa_selected_motion): finite motion, and over the sizes at
    least 50 texels of every kind: small motion, a sample on a texel centre, the Catmull-Rom centre tap on a
    k/256 + 1/512 tie in both axes, and each of the six jumps.  The tie texels are confirmed on the checker's own
    Catmull-Rom arithmetic (post_catmull_rom_axis)."""
    count = {}
    for W, H in PC.SIZES:
        c = PC.taa_case(W, H)
        assert np.isfinite(c["mv"]).all() and np.abs(c["mv"]).max() < 8
        sel = PC.taa_selected_motion(c["mv"])
        kinds = PC.taa_classify(c)
        for name, where in kinds.items():
            count[name] = count.get(name, 0) + int(where.sum())
        for y, x in zip(*np.nonzero(kinds["tie"] | kinds["centre"])):
            for tc, m, n in (((F(x) + F(0.5)) / F(W), sel[y, x, 0], W), ((F(y) + F(0.5)) / F(H), sel[y, x, 1], H)):
                sp = F(F(tc + m) * F(n))
                w, taps = PC.catmull_rom_axis(lib, sp, n)
                if kinds["tie"][y, x]:
                    assert PC.on_tie(F(F(taps[1] * F(n)) - F(0.5))), (W, H, x, y)
                else:
                    assert list(w) == [0.0, 1.0, 0.0, 0.0], (W, H, x, y)   # f = 0: all the weight on one texel
    print("TAA texels by the kind of the motion they sample with:", count)
    assert set(count) == set(PC.TAA_KINDS) and all(v >= 50 for v in count.values()), count


def test_flicker_cases_reach_both_sides(lib):
    """The flicker-mask cases: at least 5 % ones and 5 % zeros at the two largest sizes; over all sizes at least 50
    texels with dx within 1e-6 at or below 0.1 (mask 1) and 50 within 1e-6 above it (mask 0), dy below the
    threshold on both; border texels on every side; and at least 50 texels with a zero offset (normalize gives NaN,
    which min must drop)."""
    near_in = near_out = zero = 0
    for W, H in PC.SIZES:
        c = PC.flicker_case(lib, W, H)
        mask, fl, dxy = PC.flicker_mask(lib, c["z"], c["normal_w"], c["cam"])
        assert (fl[0] & 1).all() and (fl[-1] & 1).all() and (fl[:, 0] & 1).all() and (fl[:, -1] & 1).all()
        if W * H >= 300:
            assert 0.05 <= mask.mean() <= 0.95, (W, H, mask.mean())
        assert (mask[c["near_in"]] == 1).all() and (mask[c["near_out"]] == 0).all()
        assert (np.abs(dxy[c["near_in"] | c["near_out"], 0] - F(0.1)) <= PC.FLICKER_WINDOW).all()
        near_in += int(c["near_in"].sum())
        near_out += int(c["near_out"].sum())
        zero += int(((fl & 2) != 0).sum())
    print("flicker mask: within 1e-6 of 0.1 below / above, zero offsets:", near_in, near_out, zero)
    assert near_in >= 50 and near_out >= 50 and zero >= 50


def test_blur_cases_hold_their_patches():
    for W, H in PC.SIZES:
        for scale in ((1, 1), (1, 2), (2, 1)):
            z = PC.blur_case(W, H, 1, scale)["z"]
            assert z.shape == (max(1, H * scale[0] // scale[1]), max(1, W * scale[0] // scale[1]))
            if z.shape[1] >= 9 and z.shape[0] >= 3:
                assert (z == 0).sum() >= 1 and np.isinf(z).sum() >= 1 and np.isnan(z).sum() >= 1
    assert PC.largest_guard(129, 9) == 4 and PC.largest_guard(63, 3) == 1 and PC.largest_guard(1, 1) == 0
