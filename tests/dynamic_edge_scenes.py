"""The scenes and motions of the dynamic-scene edge tests (tests/test_dynamic_edges.py pins on the CPU that each one
reaches the edge it was built for; tests/test_gpu_dynamic_edges.py hands them to the kernels):

  cell_edges      triangles whose code midpoint sits exactly on a quantiser cell boundary, and one float32 below / above
  small counts    soups at the triangle counts where the LBVH launches change shape
  soup_176k       the first round count past scene_box_kernel's launch cap, the scene box pinned by the last triangles
  float classes   denormal, huge, infinite, far, collapsed and unreferenced-outlier positions of two small scenes
  subset_grid     every vertex named, 12 * nv a multiple of 256: the refit's tables follow the positions directly
  snapshot_grid   camera-facing patches of 20 .. 23 and 1027 vertices, the last one visible
"""
import dataclasses

import numpy as np

from test_bvh_refit import _motion, _scene as _refit_scene

F = np.float32
CAM = dict(pos=[0.0, 0.0, 3.0], target=[0.0, 0.0, 0.0], up=[0.0, 1.0, 0.0])


def _mk(name, p, t, flags=None, cam=CAM):
    from rsd.scenes import Scene
    t = np.ascontiguousarray(t, np.uint32).reshape(-1, 3)
    flags = np.zeros(t.shape[0], np.uint32) if flags is None else np.ascontiguousarray(flags, np.uint32)
    return Scene(name, np.ascontiguousarray(p, F).reshape(-1, 3), t, flags, cam)


# ---------------------------------------------------------------------------------------------- cell_edges

# per axis (scene box lo, hi): extents 3, 5 and 1023 have odd mantissas, so the quantiser's division is no shift
CELL_BOX = ((-1.5, 1.5), (0.0, 5.0), (-7.0, 1016.0))
# x boundary 512 is 0.0, whose float32 neighbours are +-2^-149: the definition's double subtraction mid - slo
# absorbs them (1.5 - 2^-149 rounds to 1.5).  -2^-52 is the float32 nearest below 0 that 1.5 - v resolves in double.
CELL_X0_RESOLVED = -2.0 ** -52


def cell_boundary(axis, k):
    """slo + ext * k / 1024 as a float32, asserted exact."""
    lo, hi = CELL_BOX[axis]
    num = int(lo * 1024) + int(hi - lo) * k  # the value is num / 1024 with an integer numerator
    v = F(num / 1024.0)
    assert lo * 1024 == int(lo * 1024) and abs(num) < 1 << 24 and float(v) * 1024.0 == num, (axis, k)
    return v


def cell_edges():
    """(scene, table): table rows (triangle, axis, k, which) with which = -1 / 0 / +1 for the float32 below the
    boundary k of `axis`, the boundary itself and the float32 above; which = -2 marks the extra triangle at
    CELL_X0_RESOLVED.  Each such triangle is flat on its axis (lo = hi = the value, so the tight-box midpoint is that
    float exactly) and a small right triangle inside the box on the other two.  Triangles 0 and 1 pin the scene box."""
    rng = np.random.default_rng(1024)
    lo = np.array([b[0] for b in CELL_BOX], np.float64)
    ext = np.array([b[1] - b[0] for b in CELL_BOX], np.float64)
    pos = [np.tile(F(lo), (3, 1)), np.tile(F(lo + ext), (3, 1))]
    pos[0][1, 1] += F(0.25)  # corner triangles with an area: they stay inside the box
    pos[0][2, 2] += F(0.25)
    pos[1][1, 1] -= F(0.25)
    pos[1][2, 2] -= F(0.25)
    table = []
    for axis in range(3):
        o1, o2 = (axis + 1) % 3, (axis + 2) % 3
        for k in range(1, 1024):
            b = cell_boundary(axis, k)
            vals = [(F(np.nextafter(b, F(-np.inf))), -1), (b, 0), (F(np.nextafter(b, F(np.inf))), 1)]
            if axis == 0 and k == 512:
                vals.append((F(CELL_X0_RESOLVED), -2))
            for v, which in vals:
                tri = np.empty((3, 3), F)
                tri[:, axis] = v
                a = F(lo[o1] + ext[o1] * rng.uniform(0.1, 0.8))
                c = F(lo[o2] + ext[o2] * rng.uniform(0.1, 0.8))
                tri[:, o1] = (a, F(a + F(ext[o1] / 64)), a)
                tri[:, o2] = (c, c, F(c + F(ext[o2] / 64)))
                table.append((len(pos), axis, k, which))
                pos.append(tri)
    p = np.concatenate(pos).astype(F)
    t = np.arange(p.shape[0], dtype=np.uint32).reshape(-1, 3)
    return _mk("cell_edges", p, t), np.array(table, np.int64)


def axis_codes(code, axis):
    """The 10-bit axis code out of lbvh_checker.codes' 30-bit Morton codes (x in the highest bit of each triple)."""
    code = np.asarray(code, np.uint64)
    q = np.zeros(code.shape, np.int64)
    for bit in range(10):
        q |= (((code >> np.uint64(3 * bit + 2 - axis)) & np.uint64(1)).astype(np.int64)) << bit
    return q


# ---------------------------------------------------------------------------------------------- soups

# 2 .. 4: the leaf root with cnt > 1; 6 .. 9 and 17 .. 21: a root half first exceeds 4 and splits again;
# 64 .. 66 and 256 .. 258: ni = nt - 1 crosses a wave and a block
SMALL_COUNTS = [2, 3, 4, 6, 9, 17, 21, 64, 65, 66, 256, 257, 258]


def soup(nt, spread=1.0, size=0.3, seed=None, share=True):
    """tests/native/check_lbvh.cpp's soup: a centroid per triangle in [-spread, spread]^3, its vertices within `size`
    of it; two vertices are shared between triangles (which leaves two vertices that no triangle names)."""
    rng = np.random.default_rng(nt if seed is None else seed)
    c = spread * rng.uniform(-1.0, 1.0, (nt, 1, 3))
    p = (c + size * rng.uniform(-1.0, 1.0, (nt, 3, 3))).astype(F).reshape(-1, 3)
    t = np.arange(3 * nt, dtype=np.uint32)
    if share and nt >= 2:
        t[3] = t[0]
    if share and nt >= 3:
        t[7] = t[2]
    flags = (np.arange(nt, dtype=np.uint32) * np.uint32(2654435761)) >> np.uint32(30)
    return _mk(f"soup_{nt}", p, t.reshape(-1, 3), flags)


def jitter(scene, seed=3, amount=0.05):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(scene.positions + (amount * rng.standard_normal(scene.positions.shape)).astype(F), F)


BOX_CAP = 2048 * 256  # csrc/lbvh.hip scene_box_kernel: at most 2048 blocks of 256 lanes, one index component each
BIG_NT = 176_000


def soup_176k(every=1):
    """176 000 small triangles, centroids in [-10, 10]^3; the last six triangles each carry one extreme of the scene
    box (+-12 on one axis), so the index components that define the box lie past BOX_CAP: only lanes on their second
    trip through scene_box_kernel's loop read them.  every = 16: each 16th of the ordinary triangles plus the same
    last six -- the subsample the numpy checker is run on."""
    nt = BIG_NT
    rng = np.random.default_rng(176)
    c = rng.uniform(-10.0, 10.0, (nt, 1, 3))
    p = (c + 0.05 * rng.uniform(-1.0, 1.0, (nt, 3, 3))).astype(F)
    for j in range(6):
        p[nt - 6 + j, 0, j % 3] = F(12.0 if j >= 3 else -12.0)
    if every > 1:
        p = np.concatenate([p[:nt - 6:every], p[nt - 6:]])
    n = p.shape[0]
    return _mk("soup_176k" if every == 1 else f"soup_176k_every_{every}", p.reshape(-1, 3),
               np.arange(3 * n, dtype=np.uint32).reshape(-1, 3))


def box_defining_components(scene):
    """Positions in the flat index buffer of the components that name a vertex holding an extreme of the scene box."""
    p = scene.positions[scene.indices.reshape(-1)]  # [3 nt, 3]
    at = (p == p.min(axis=0)) | (p == p.max(axis=0))
    return np.flatnonzero(at.any(axis=1)), at


# ---------------------------------------------------------------------------------------------- float classes

FLOAT_BASES = ["soup_400", "grid_24"]
FLOAT_CLASSES = ["denormal_mixed_sign", "huge", "one_infinite", "far_outside", "collapsed", "unreferenced_outliers"]
FINITE_CLASSES = ["denormal_mixed_sign", "huge", "far_outside", "collapsed"]  # these are also rendered
OUTLIERS = 3


def float_base(name):
    if name == "soup_400":  # |coordinates| up to 25.3: times 1e37 the extent passes FLT_MAX, the coordinates do not
        return soup(400, spread=25.0, seed=22)
    return _refit_scene(name)


def float_class(base, cls):
    """(the ordinary scene to upload, the positions of the class).  unreferenced_outliers needs three vertices more
    than the base: the ordinary scene carries them at the origin, named by no triangle and last in the buffer."""
    s = float_base(base)
    if cls == "unreferenced_outliers":
        p0 = np.concatenate([s.positions, np.zeros((OUTLIERS, 3), F)])
        s = dataclasses.replace(s, positions=np.ascontiguousarray(p0, F))
        p = s.positions.copy()
        p[-3], p[-2], p[-1] = F(1e30), F(-1e30), F(np.nan)
        return s, p
    if cls == "huge":
        return s, np.ascontiguousarray(s.positions * F(1e37), F)
    if cls == "one_infinite":
        p = s.positions.copy()
        p[s.indices[1][1], 1] = F(np.inf)
        return s, p
    return s, np.ascontiguousarray(_motion(cls, s), F)


def referenced_nan(base="soup_400"):
    """One coordinate of a vertex a triangle names is NaN (the positive quiet NaN: the highest key of bvh_refit.h)."""
    s = float_base(base)
    p = s.positions.copy()
    p[s.indices[5][2], 0] = F(np.nan)
    return s, p


# ---------------------------------------------------------------------------------------------- update_subset

SUBSET_NX, SUBSET_NY = 20, 16


def subset_grid():
    """A 20 x 16 height field: 320 vertices (a multiple of 64; 12 * 320 = 15 * 256), every one named by a triangle."""
    rng = np.random.default_rng(320)
    xs, ys = np.meshgrid(np.linspace(-2.0, 2.0, SUBSET_NX), np.linspace(-1.5, 1.5, SUBSET_NY))
    p = np.stack([xs.ravel(), ys.ravel(), rng.uniform(-0.3, 0.3, xs.size)], 1).astype(F)
    i = np.arange(xs.size).reshape(SUBSET_NY, SUBSET_NX)
    a, b, c, d = i[:-1, :-1], i[:-1, 1:], i[1:, 1:], i[1:, :-1]
    t = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 2).reshape(-1, 3)
    return _mk("subset_grid", p, t)


# ---------------------------------------------------------------------------------------------- motion snapshot

SNAPSHOT_NV = [20, 21, 22, 23, 1027]


def snapshot_grid(nv):
    """A patch facing the camera at (0, 0, 3): a grid (5 x 4, or 32 x 32 for 1027) in the plane z ~ 0 plus nv - grid
    further vertices to its right, each the apex of a triangle on two vertices of the grid's right edge.  Double-sided.
    The last vertex of the buffer always belongs to a triangle."""
    nx, ny = (32, 32) if nv > 1000 else (5, 4)
    extra = nv - nx * ny
    assert 0 <= extra < ny
    rng = np.random.default_rng(nv)
    xs, ys = np.meshgrid(np.linspace(-0.9, 0.5, nx), np.linspace(-0.6, 0.6, ny))
    p = np.stack([xs.ravel(), ys.ravel(), rng.uniform(-0.05, 0.05, xs.size)], 1)
    i = np.arange(nx * ny).reshape(ny, nx)
    a, b, c, d = i[:-1, :-1], i[:-1, 1:], i[1:, 1:], i[1:, :-1]
    t = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 2).reshape(-1, 3)
    step = (ny - 1) // 3  # the apex triangles span a third of the edge each: tall enough to own pixels
    for j in range(extra):
        lo, hi = i[j * step, -1], i[(j + 1) * step, -1]
        apex = [0.8, 0.5 * (p[lo, 1] + p[hi, 1]), 0.02 * (j + 1)]
        t = np.concatenate([t, [[lo, nx * ny + j, hi]]])
        p = np.concatenate([p, [apex]])
    s = _mk(f"snapshot_{nv}", p, t, flags=np.ones(t.shape[0], np.uint32))
    assert s.positions.shape[0] == nv and (s.indices == nv - 1).any()
    return s


def snapshot_motion(scene):
    """(P1, P2): P1 moves every coordinate of every vertex away from the upload's (a stale dword of the snapshot is
    then a different number), P2 moves on a little."""
    rng = np.random.default_rng(scene.positions.shape[0] + 1)
    p1 = scene.positions + F([0.15, -0.1, 0.4]) + (0.02 * rng.standard_normal(scene.positions.shape)).astype(F)
    p2 = p1 + F([0.05, 0.04, -0.1]) + (0.01 * rng.standard_normal(scene.positions.shape)).astype(F)
    return np.ascontiguousarray(p1, F), np.ascontiguousarray(p2, F)
