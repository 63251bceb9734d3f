"""GPU edge cases of the post-AO image passes (csrc/post.hip) against the scalar checker of tests/post_checker.py,
bit for bit: frames on the edges of the 64 x 4 workgroup, frames narrower than the blur radius and the dilation ring,
reprojections exactly on the guard-band limits, bilinear ties, the 10 % depth test on its threshold, every texel
format of ImageEquation and of Deinterleave / Interleave.  Every output buffer carries 64 texels of sentinel before
and after it and is pre-filled with the sentinel: nothing outside the scissor or the extent may change.
tests/test_post_checker.py shows on the checker alone that the inputs reach the branches they are meant to reach."""
import ctypes as C

import numpy as np
import pytest

import post_checker as PC

pytestmark = pytest.mark.gpu
F = np.float32
S, PAD = PC.SENTINEL, PC.PAD


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return PC.build(tmp_path_factory.mktemp("post_ref"))


@pytest.fixture(scope="module")
def rsd():
    from rsd import abi
    return abi


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()   # a copy: the shared cases are read-only


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Padded:
    """An output buffer of `shape` texels of `dtype` between two runs of PAD sentinel texels, sentinel-filled."""

    def __init__(self, torch, shape, dtype=np.uint8):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.texel = int(np.prod(self.shape[2:], dtype=np.int64)) * self.dtype.itemsize   # texel = trailing dims
        self.n = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.pad = PAD * max(self.texel, 16)   # a multiple of 16: the payload stays aligned for the widest texel
        self.buf = torch.full((self.n + 2 * self.pad,), S, dtype=torch.uint8, device="cuda")
        self.ptr = C.c_void_p(self.buf.data_ptr() + self.pad)

    def get(self):
        """The payload; asserts the padding untouched."""
        raw = self.buf.cpu().numpy()
        assert (raw[:self.pad] == S).all() and (raw[self.pad + self.n:] == S).all(), "write outside the buffer"
        return raw[self.pad:self.pad + self.n].view(self.dtype).reshape(self.shape)


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype == np.float32:
        nan = np.isnan(want)
        return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    return np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ blur

def _run_blur(torch, rsd, lib, c, W, H, guard, radius, better):
    src, z = c["src"], c["z"]
    texel = 1 if src.ndim == 2 else src.shape[2]
    ds, dz = _dev(torch, src), _dev(torch, z)
    pp, out = Padded(torch, (H, W)), Padded(torch, (H, W))
    rsd.check(rsd.lib().rsd_cross_bilateral_blur_src(_ptr(ds), texel, _ptr(dz), z.shape[1], z.shape[0], pp.ptr, out.ptr,
                                                     W, H, guard, radius, int(better), _stream(torch)), "blur")
    torch.cuda.synchronize()
    want, want_pp = PC.blur(lib, src, z, guard, radius, better)
    assert np.array_equal(pp.get(), want_pp), ("ping-pong", W, H, guard, radius, better)
    assert np.array_equal(out.get(), want), (W, H, guard, radius, better)
    return want


@pytest.mark.parametrize("W,H", PC.SIZES + [(9, 7)])
def test_blur_sizes_radii_slopes_guards(torch, rsd, lib, W, H):
    """Radius 1, 4 and 20 (at 9 x 7 and the small frames every far tap is the clamped edge texel), both slopes, guard
    0, 3 and the largest that leaves a one-pixel scissor; depth patches of 0, +inf and NaN as centre and side taps."""
    c = PC.blur_case(W, H)
    guards = sorted({g for g in (0, 3, PC.largest_guard(W, H)) if 2 * g < min(W, H)})
    for guard in guards:
        for radius in (1, 4, 20):
            for better in (True, False):
                _run_blur(torch, rsd, lib, c, W, H, guard, radius, better)


@pytest.mark.parametrize("scale", [(1, 2), (2, 1)])
@pytest.mark.parametrize("texel", [1, 2])
def test_blur_depth_of_another_size_and_two_byte_source(torch, rsd, lib, scale, texel):
    """z_w / z_h at half and at double the AO image's size; src_texel_bytes 1 and 2 (the dualAO map's first byte)."""
    for W, H in ((65, 5), (129, 9)):
        c = PC.blur_case(W, H, texel, scale)
        assert c["z"].shape != (H, W)
        for radius, better, guard in ((4, True, 0), (20, False, 2)):
            _run_blur(torch, rsd, lib, c, W, H, guard, radius, better)
    c = PC.blur_case(65, 5, texel, (1, 1))
    _run_blur(torch, rsd, lib, c, 65, 5, 1, 4, True)


# ------------------------------------------------------------------------------------------------ de/interleave

@pytest.mark.parametrize("texel", [1, 2, 4, 8, 16])
def test_deinterleave_interleave_every_residue_and_texel_size(torch, rsd, lib, texel):
    """All sixteen (W mod 4, H mod 4) at sizes around 8 and around 64, and the six frame sizes of the module; the
    2-byte texel is the dualAO map."""
    rng = np.random.default_rng(texel)
    sizes = [(W, H) for W0, H0 in ((5, 5), (61, 62)) for W in range(W0, W0 + 4) for H in range(H0, H0 + 4)]
    for W, H in sizes + PC.SIZES:   # ... and the frames on the workgroup's edges, 1 x 1 among them
        a = rng.integers(1, 256, (H, W, texel)).astype(np.uint8)
        src = _dev(torch, a)
        want = PC.deinterleave(lib, a)
        dst = Padded(torch, want.shape)
        rsd.check(rsd.lib().rsd_deinterleave(_ptr(src), W, H, texel, dst.ptr, _stream(torch)), "deinterleave")
        back = Padded(torch, a.shape)
        rsd.check(rsd.lib().rsd_interleave(dst.ptr, W, H, texel, back.ptr, _stream(torch)), "interleave")
        torch.cuda.synchronize()
        assert np.array_equal(dst.get(), want), (W, H, texel)
        assert np.array_equal(back.get(), a), (W, H, texel)


# ------------------------------------------------------------------------------------------------ TemporalAO

@pytest.mark.parametrize("W,H", PC.SIZES + [(67, 19)])
def test_temporal_ao_limits_thresholds_and_ties(torch, rsd, lib, W, H):
    """Guard 0 and 5 (5 where the frame admits it: 67 x 19), with a stable mask and with none: reprojections exactly
    on uvMin / uvMax and one float to either side, the depth test next to 0.1 on both sides, current and previous
    depth 0, history counts 0, 29, 30 and 255, bilinear ties and exact texel centres."""
    cam, _ = PC.cameras(129, 9)
    for guard in (0, 5):
        if 2 * guard >= min(W, H):
            continue
        for use_mask in (False, True):
            c = PC.tao_case(lib, W, H, guard, use_mask, cam)
            d = {k: _dev(torch, c[k]) for k in ("ao", "z", "mv", "prev_z", "prev_ao", "prev_n")}
            dm = _dev(torch, c["mask"]) if use_mask else None
            out, hist = Padded(torch, (H, W)), Padded(torch, (H, W))
            m = np.ascontiguousarray(c["m"], F)
            rsd.check(rsd.lib().rsd_temporal_ao(_ptr(d["ao"]), _ptr(d["z"]), _ptr(d["mv"]), _ptr(d["prev_z"]),
                                                _ptr(d["prev_ao"]), _ptr(d["prev_n"]), _ptr(dm), W, H, guard,
                                                C.byref(cam), m.ctypes.data_as(C.c_void_p), out.ptr, hist.ptr,
                                                _stream(torch)), "rsd_temporal_ao")
            torch.cuda.synchronize()
            want, want_n, _, _ = PC.temporal_ao(lib, c["ao"], c["z"], c["mv"], c["prev_z"], c["prev_ao"], c["prev_n"],
                                                c["mask"], guard, cam, c["m"])
            assert np.array_equal(hist.get(), want_n), (W, H, guard, use_mask)
            assert np.array_equal(out.get(), want), (W, H, guard, use_mask)


# ------------------------------------------------------------------------------------------------ TAA

@pytest.mark.parametrize("W,H", PC.SIZES)
def test_taa_wrap_jumps_and_centres(torch, rsd, lib, W, H):
    """sigma 0.5 and 4, anti-flicker on and off, a first frame with zero history and a second one; bands of small motion,
    of motion onto texel centres, of motion that puts the Catmull-Rom centre tap on bilinear ties, and of jumps of
    +-0.6, +-1.3 and +-7.25 images (the longest vector of each 3 x 3 neighbourhood is of the band's kind).  Motion vectors stay finite: a float -> int conversion of
    inf or NaN is undefined in C, so the checker cannot define the wrapped index of such a tap."""
    for first in (True, False):
        c = PC.taa_case(W, H, first_frame=first)
        col, mv, prev = (_dev(torch, c[k]) for k in ("color", "mv", "prev"))
        for sigma, anti in ((0.5, True), (4.0, False), (4.0, True), (0.5, False)):
            out = Padded(torch, (H, W, 4), np.float32)
            rsd.check(rsd.lib().rsd_taa(_ptr(col), _ptr(mv), _ptr(prev), W, H, 0.1, sigma, int(anti), out.ptr,
                                        _stream(torch)), "rsd_taa")
            torch.cuda.synchronize()
            want = PC.taa(lib, c["color"], c["mv"], c["prev"], 0.1, sigma, anti)
            assert _same_bits(out.get(), want), (W, H, first, sigma, anti)


# ------------------------------------------------------------------------------------------------ mask, dilation

@pytest.mark.parametrize("W,H", PC.SIZES)
def test_flicker_mask_borders_and_threshold(torch, rsd, lib, W, H):
    """Border rows and columns (one neighbour loads 0), equal neighbouring view positions (normalize of a zero vector
    meets min), |dot| on both sides of 0.1; the mask then goes through the dilation with min and with max."""
    c = PC.flicker_case(lib, W, H)
    dz, dn = _dev(torch, c["z"]), _dev(torch, c["normal_w"])
    mask = Padded(torch, (H, W))
    rsd.check(rsd.lib().rsd_ao_flicker_mask(_ptr(dz), _ptr(dn), W, H, C.byref(c["cam"]), mask.ptr, _stream(torch)),
              "rsd_ao_flicker_mask")
    torch.cuda.synchronize()
    want = PC.flicker_mask(lib, c["z"], c["normal_w"], c["cam"])[0]
    assert np.array_equal(mask.get(), want), (W, H)
    for op in (0, 1):
        out = Padded(torch, (H, W))
        rsd.check(rsd.lib().rsd_binary_dilation(mask.ptr, W, H, op, out.ptr, _stream(torch)), "rsd_binary_dilation")
        torch.cuda.synchronize()
        assert np.array_equal(out.get(), PC.binary_dilation(lib, want, op)), (W, H, op)


@pytest.mark.parametrize("W,H", [(1, 1), (2, 3), (5, 4)])
def test_dilation_ring_wraps_past_the_image(torch, rsd, lib, W, H):
    """Frames smaller than the radius-2 ring: every Gather wraps, some more than once around."""
    rng = np.random.default_rng(W * 10 + H)
    for trial in range(4):
        m = (rng.random((H, W)) < (0.3 if trial % 2 else 0.7)).astype(np.uint8) * (1 + trial)
        dm = _dev(torch, m)
        for op in (0, 1):
            out = Padded(torch, (H, W))
            rsd.check(rsd.lib().rsd_binary_dilation(_ptr(dm), W, H, op, out.ptr, _stream(torch)), "rsd_binary_dilation")
            torch.cuda.synchronize()
            assert np.array_equal(out.get(), PC.binary_dilation(lib, m, op)), (W, H, op, trial)


# ------------------------------------------------------------------------------------------------ ImageEquation

def _run_equation(torch, rsd, formula, inputs, W, H, out_fmt):
    tex = (rsd.Texture * 4)()
    keep = []
    for k, (img, fmt) in enumerate(inputs):
        if img is not None:
            t = _dev(torch, img)
            keep.append(t)
            tex[k] = rsd.Texture(t.data_ptr(), img.shape[1], img.shape[0], 1, fmt, t.numel() * t.element_size())
    h = C.c_void_p()
    rsd.check(rsd.lib().rsd_image_equation_compile(formula.encode(), C.byref(h)), formula)
    ch = {PC.RGBA32F: 4, PC.RG32F: 2, PC.R32F: 1, PC.R8UNORM: 1}[out_fmt]
    out = Padded(torch, (H, W, ch), np.uint8 if out_fmt == PC.R8UNORM else np.float32)
    ot = rsd.Texture(out.ptr.value, W, H, 1, out_fmt, out.n)
    rsd.check(rsd.lib().rsd_image_equation_run(h, tex, C.byref(ot), _stream(torch)), formula)
    torch.cuda.synchronize()
    rsd.lib().rsd_image_equation_release(h)
    return out.get()


@pytest.mark.parametrize("out_fmt", [PC.RGBA32F, PC.RG32F, PC.R32F, PC.R8UNORM])
def test_image_equation_formats_functions_and_stack(torch, rsd, lib, out_fmt):
    """All eight input formats (inputs smaller and larger than the output), all four output formats, every function,
    dot of 2, 3 and 4 lanes, a program at stack depth 8.  Bit for bit, except on texels the checker marks fragile
    (a double transcendental whose two neighbouring doubles do not round to the same float: device and host libm
    may differ by one double ulp), where the GPU must equal one of the three candidates."""
    for W, H in PC.SIZES:
        images = PC.image_inputs(W, H)
        for formula, names in PC.EQUATIONS:
            inputs = [images[k] if k else (None, 0) for k in names]
            if out_fmt == PC.R8UNORM:
                formula = PC.unorm_formula(formula)   # into [0, 1): the stored byte is not pinned at 255
            got = _run_equation(torch, rsd, formula, inputs, W, H, out_fmt)
            cands, fragile = PC.image_equation(formula, inputs, W, H)
            stored = [PC.store(lib, c, out_fmt).reshape(got.shape) for c in cands]
            solid = ~fragile
            assert _same_bits(got[solid], stored[1][solid]), (formula, W, H)
            for y, x in zip(*np.nonzero(fragile)):
                assert any(_same_bits(got[y, x], s[y, x]) for s in stored), (formula, x, y)


def test_image_equation_refuses_depth_nine(rsd):
    h = C.c_void_p()
    assert rsd.lib().rsd_image_equation_compile(PC.DEPTH9.encode(), C.byref(h)) == rsd.ERR_INVALID_ARG and not h.value


# ------------------------------------------------------------------------------------------------ RayMinMaxLength

@pytest.mark.parametrize("W,H", PC.SIZES)
def test_ray_min_max_length_sizes_and_specials(torch, rsd, lib, W, H):
    """Random interval words with rayMax == 0, inverted intervals, +-inf, NaN, a denormal and -0 among them."""
    rmin, rmax = PC.ray_case(W, H)
    dmn, dmx = _dev(torch, rmin.view(np.int32)), _dev(torch, rmax.view(np.int32))
    out = Padded(torch, (H, W), np.float32)
    rsd.check(rsd.lib().rsd_ray_min_max_length(_ptr(dmn), _ptr(dmx), W, H, out.ptr, _stream(torch)), "ray length")
    torch.cuda.synchronize()
    assert _same_bits(out.get(), PC.ray_min_max_length(lib, rmin, rmax)), (W, H)


# ------------------------------------------------------------------------------------------------ motion vectors

@pytest.mark.parametrize("W,H", PC.SIZES)
def test_motion_vectors_both_entries(torch, rsd, lib, W, H):
    """A translation, a rotation, both, and a previous camera with every point behind it ((2, 2)); the linear-depth
    entry with the background at farZ, the raster entry with the background decided on the raw depth at exactly 1.0
    and one float below it (near 0.1 / far 10, where the linearised 1.0 lands below farZ)."""
    rng = np.random.default_rng(W + H)
    for raw, (near, far) in ((False, (0.1, 1000.0)), (True, (0.1, 10.0))):
        cur, prevs = PC.cameras(W, H, near, far)
        if raw:
            z = rng.uniform(0.5, 0.99, (H, W)).astype(F)
            z.reshape(-1)[::5] = 1.0
            z.reshape(-1)[2::5] = np.nextafter(F(1), F(0))
        else:
            z = (2.0 + 28.0 * rng.random((H, W))).astype(F)
            z.reshape(-1)[::5] = cur.farZ
            z.reshape(-1)[2::5] = np.nextafter(F(cur.farZ), F(0))
        dz = _dev(torch, z)
        fn = rsd.lib().rsd_motion_vectors_raster if raw else rsd.lib().rsd_motion_vectors
        for name, prev in prevs.items():
            out = Padded(torch, (H, W, 2), np.float32)
            rsd.check(fn(C.byref(cur), C.byref(prev), _ptr(dz), W, H, out.ptr, _stream(torch)), name)
            torch.cuda.synchronize()
            want, _ = PC.motion_vectors(lib, cur, prev, z, raw=raw)
            got = out.get()
            assert _same_bits(got, want), (W, H, raw, name)
            assert (got.reshape(-1, 2)[::5] == 0).all()
            if name == "behind" and not raw:
                assert (got.reshape(-1, 2)[2::5] == 2).all()
