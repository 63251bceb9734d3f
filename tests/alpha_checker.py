"""An independent numpy float32 restatement of the whole alpha decision (DESIGN.md "Alpha test"): the barycentric
texture coordinate, the ray-cone level, the LOD clamp and its 8-bit fraction, the box mip chain, the wrap-addressed
bilinear tap with 8 sub-texel bits, the trilinear blend and the float16 threshold.  It shares no code with the oracle
(oracle/rsd_oracle.c), the device (csrc/alpha_test.h, csrc/tex_sample.h) or the host upload (csrc/rsd_host.cpp): every
float expression is written out here, rounded operation by operation in float32, log2 in double rounded once.

value() works on arrays of hit tuples (prim, bu, bv, t, d) and reports, per tuple, which of EDGES it reached;
tests/test_alpha_edges.py counts them on the frames that tests/test_gpu_alpha_edges.py renders.  The scalar helpers
(texel, bilinear, mips, lod_split) are the ones tests/test_alpha.py pins the oracle with."""
import numpy as np

F = np.float32
NO_TEXTURE = 0xFFFFFFFF

# the edges a sample can reach
EDGES = ("carry_x", "carry_y", "carry_lod",      # a fraction that rounds to 256 / 256 carries into the next texel / mip
         "tap_left", "tap_right",                # a tap at an index < 0 / >= n before wrapping, with non-zero weight
         "tap_above", "tap_below",
         "one_texel_x", "one_texel_y",           # the sampled mip is 1 texel wide / high (every tap wraps onto it)
         "lod_clamped_low", "lod_clamped_high",  # level < 0 / level > mips - 1
         "qf_zero",                              # LOD fraction 0: one bilinear tap
         "last_mip",                             # l0 + 1 == mips: one bilinear tap of the 1 x 1 mip
         "blend")                                # two bilinear taps blended


# ---- scalars (tests/test_alpha.py)

def half(threshold):
    """MaterialHeader keeps the threshold as float16 (round to nearest even), widened again."""
    with np.errstate(over="ignore", invalid="ignore"):
        return F(np.float16(F(threshold)))


def texel(tex, x, y):
    h, w = tex.shape
    return F(tex[y % h, x % w]) / F(255.0)


def bilinear(tex, u, v):
    """One tap of one mip at (u, v), scalars."""
    return _bilinear(np.asarray(tex), np.array([u], F), np.array([v], F))[0]


def mips(tex):
    """The box chain down to 1 x 1: (a + b + c + d + 2) / 4 over 2 x 2 texels clamped to the level."""
    chain = [np.asarray(tex).astype(np.int64)]
    while chain[-1].shape != (1, 1):
        a = chain[-1]
        h, w = a.shape
        nh, nw = max(1, h // 2), max(1, w // 2)
        ys, xs = np.arange(nh), np.arange(nw)
        y0, y1 = np.minimum(2 * ys, h - 1), np.minimum(2 * ys + 1, h - 1)
        x0, x1 = np.minimum(2 * xs, w - 1), np.minimum(2 * xs + 1, w - 1)
        s = a[y0][:, x0] + a[y0][:, x1] + a[y1][:, x0] + a[y1][:, x1]
        chain.append((s + 2) // 4)
    return [c.astype(np.uint8) for c in chain]


def lod_split(level, mip_count):
    """(l0, qf) of a level: NaN gives 0, clamp to [0, mips - 1], 8 fraction bits with the carry."""
    l0, qf, _ = _lod_split(np.array([level], F), mip_count)
    return int(l0[0]), F(qf[0])


# ---- arrays

def _split(x):
    """x = i + q / 256, q in 0 .. 255; (i, q, carried)."""
    f0 = np.floor(x)
    q = np.floor((x - f0) * F(256.0) + F(0.5))
    i = f0.astype(np.int64)
    carry = q >= F(256.0)
    return i + carry, np.where(carry, F(0.0), q).astype(F), carry


def _bilinear(tex, u, v, edges=None, sel=None):
    """The value of one mip `tex` at arrays (u, v); edges: dict name -> bool array to OR into at index sel."""
    h, w = tex.shape
    ix, qx, cx = _split(u * F(w) - F(0.5))
    iy, qy, cy = _split(v * F(h) - F(0.5))
    wx, wy = qx * F(1.0 / 256.0), qy * F(1.0 / 256.0)
    t = tex.astype(F) / F(255.0)
    x0, x1, y0, y1 = ix % w, (ix + 1) % w, iy % h, (iy + 1) % h
    one = F(1.0)
    r0 = t[y0, x0] * (one - wx) + t[y0, x1] * wx
    r1 = t[y1, x0] * (one - wx) + t[y1, x1] * wx
    out = r0 * (one - wy) + r1 * wy
    if edges is not None:
        # on the indices BEFORE wrapping: a tap at a negative index (where a C `%` alone goes wrong) or at n and
        # beyond, counted when its weight is not zero (the left tap's 1 - w never is)
        left, right = ix < 0, (ix >= w) | ((ix + 1 >= w) & (qx != 0))
        above, below = iy < 0, (iy >= h) | ((iy + 1 >= h) & (qy != 0))
        for name, m in (("carry_x", cx), ("carry_y", cy),
                        ("tap_left", left), ("tap_right", right), ("tap_above", above), ("tap_below", below),
                        ("one_texel_x", np.full(u.shape, w == 1)), ("one_texel_y", np.full(u.shape, h == 1))):
            edges[name][sel] |= m
    return out.astype(F)


def _lod_split(level, mip_count):
    top = F(mip_count - 1)
    nan = level != level
    lod = np.where(nan, F(0.0), level).astype(F)
    low, high = lod < F(0.0), lod > top
    lod = np.where(low, F(0.0), np.where(high, top, lod)).astype(F)
    l0, qf, carry = _split(lod)
    return l0, qf, dict(lod_clamped_low=low & ~nan, lod_clamped_high=high, carry_lod=carry)


def sample(chain, u, v, level):
    """SampleLevel(uv, level) of a mip chain (mips()) at arrays: (alpha, edges, l0)."""
    n = u.shape[0]
    edges = {k: np.zeros(n, bool) for k in EDGES}
    l0, qf, e = _lod_split(level, len(chain))
    for k, m in e.items():
        edges[k] |= m
    single = (qf == 0) | (l0 + 1 >= len(chain))
    edges["qf_zero"] |= qf == 0
    edges["last_mip"] |= l0 + 1 == len(chain)
    edges["blend"] |= ~single
    out = np.zeros(n, F)
    f = qf * F(1.0 / 256.0)
    for l in np.unique(l0):
        sel = np.flatnonzero(l0 == l)
        s0 = _bilinear(chain[l], u[sel], v[sel], edges, sel)
        two = ~single[sel]
        if two.any():
            s2 = sel[two]
            s1 = _bilinear(chain[l + 1], u[s2], v[s2], edges, s2)
            s0[two] = s0[two] * (F(1.0) - f[s2]) + s1 * f[s2]
        out[sel] = s0
    return out, edges, l0


def interpolate_uv(uv6, bu, bv):
    """Scene::computeVertexData's texture coordinate: three products summed in order, each rounded.  uv6: [n, 6] =
    (u0, v0, u1, v1, u2, v2) of the hit's triangle."""
    bu, bv = np.asarray(bu, F), np.asarray(bv, F)
    b0 = F(1.0) - bu - bv
    tu = uv6[:, 0] * b0 + uv6[:, 2] * bu + uv6[:, 4] * bv
    tv = uv6[:, 1] * b0 + uv6[:, 3] * bu + uv6[:, 5] * bv
    return tu.astype(F), tv.astype(F)


def _log2_once(x):
    """log2 in double of a float32 array, rounded to float32 once."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log2(x.astype(np.float64)).astype(F)


def ray_cone_level(tri9, tex_w, tex_h, t, d, spread):
    """0.5 log2(w h) + log2(|spread t| / |d . n|): tri9 [n, 9] the hit triangles' vertices, t [n], d [n, 3]."""
    v0, v1, v2 = tri9[:, 0:3].astype(F), tri9[:, 3:6].astype(F), tri9[:, 6:9].astype(F)
    e1, e2 = v1 - v0, v2 - v0
    cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                   e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1).astype(F)
    dot = lambda a, b: a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]  # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F(1.0) / np.sqrt(dot(cr, cr))
        n = cr * inv[:, None]
        width = F(spread) * np.asarray(t, F) + F(0.0)
        lam = F(0.0) + _log2_once(np.abs(width) / np.abs(dot(np.asarray(d, F), n)))
    dims = F(np.uint32(tex_w) * np.uint32(tex_h))
    return (F(0.5) * F(np.log2(np.float64(dims))) + lam).astype(F)


class Checker:
    """The alpha decision of a scene (rsd.scenes.Scene with .alpha) on hit tuples."""

    def __init__(self, scene):
        a = scene.alpha
        self.scene = scene
        self.chains = [mips(t) for t in a.textures]
        self.thresholds = np.array([half(t) for t in a.thresholds], F)
        ind = np.asarray(scene.indices, np.int64)
        self.uv6 = np.asarray(a.texcoords, F)[ind].reshape(-1, 6)
        self.tri9 = np.asarray(scene.positions, F)[ind].reshape(-1, 9)

    def value(self, prim, bu, bv, t=None, d=None, spread=None):
        """(alpha, edges, detail) of the tuples; t, d, spread given: the ray-cone LOD, else LOD 0.  detail: dict with
        l0 (the first mip read, -1 without a texture) and tex (the texture, -1 without)."""
        a = self.scene.alpha
        prim = np.asarray(prim, np.int64)
        n = prim.shape[0]
        mat = np.asarray(a.tri_material, np.int64)[prim]
        tex = np.asarray(a.material_textures, np.int64)[mat]
        out = np.asarray(a.alphas, F)[mat].copy()
        edges = {k: np.zeros(n, bool) for k in EDGES}
        l0 = np.full(n, -1, np.int64)
        tu, tv = interpolate_uv(self.uv6[prim], bu, bv)
        for ti in np.unique(tex[tex != NO_TEXTURE]):
            sel = np.flatnonzero(tex == ti)
            chain = self.chains[ti]
            h, w = chain[0].shape
            if t is None:
                level = np.zeros(sel.size, F)
            else:
                level = ray_cone_level(self.tri9[prim[sel]], w, h, np.asarray(t, F)[sel], np.asarray(d, F)[sel], spread)
            val, e, l = sample(chain, tu[sel], tv[sel], level)
            out[sel] = val
            l0[sel] = l
            for k in EDGES:
                edges[k][sel] = e[k]
        return out, edges, dict(l0=l0, tex=np.where(tex == NO_TEXTURE, -1, tex), mat=mat)

    def kept(self, alpha, mat):
        """evalBasicAlphaTest: the hit is discarded when alpha < threshold (false for a NaN on either side)."""
        with np.errstate(invalid="ignore"):
            return ~(alpha < self.thresholds[mat])
