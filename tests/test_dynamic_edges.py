"""CPU: the inputs of tests/test_gpu_dynamic_edges.py are the ones meant (tests/dynamic_edge_scenes.py).

For every scene and motion two things: the host definitions the GPU tests compare with (rsd_bvh_build_lbvh,
rsd_bvh_refit) equal the independent numpy checkers byte for byte, and an assertion shows that the input reaches the
edge it was built for -- a cell boundary of the quantiser, a launch shape of the LBVH kernels, the second trip of
scene_box_kernel's loop, a float class.  Where a checker is no reference (a NaN a triangle names: numpy's min / max
propagate it, the shared headers order it by key) the comparison is left out and the test says so."""
import dataclasses

import numpy as np
import pytest

import dynamic_edge_scenes as E
import lbvh_checker
import mvec_checker as MV
from bvh_refit_checker import EMPTY, expected_refit, layout
from lbvh_checker import expected_lbvh

FLT_MAX = float(np.finfo(np.float32).max)
TINY = float(np.finfo(np.float32).tiny)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _lbvh_equals_checker(scene, positions=None):
    from rsd.frame import host_bvh_lbvh
    s = scene if positions is None else dataclasses.replace(scene, positions=positions)
    bvh, off = host_bvh_lbvh(s)
    want, woff, _ = expected_lbvh(s.positions, s.indices, s.flags)
    bad = np.flatnonzero(_u32(bvh) != want) if bvh.nbytes == want.nbytes else np.arange(1)
    assert off == woff and bad.size == 0, (scene.name, off, woff, bad.size, bad[:8])
    return bvh, off


# ---------------------------------------------------------------------------------------------- cell_edges

@pytest.fixture(scope="module")
def cells():
    scene, table = E.cell_edges()
    return scene, table, lbvh_checker.codes(scene.positions, scene.indices)


def test_cell_edges_boundaries_are_exact_floats_inside_the_pinned_box(cells):
    scene, table, _ = cells
    nt = scene.indices.shape[0]
    assert nt == 2 + 3 * 3 * 1023 + 1 and scene.positions.shape[0] == 3 * nt
    used = scene.positions[scene.indices.reshape(-1)]
    for axis, (lo, hi) in enumerate(E.CELL_BOX):
        assert used[:, axis].min() == lo and used[:, axis].max() == hi, "the corner triangles pin the scene box"
        ext = hi - lo
        assert np.frexp(ext)[0] != 0.5, "an extent that is a power of two would make the division a shift"
        for k in range(1, 1024):
            v = E.cell_boundary(axis, k)  # asserts the numerator is an integer below 2^24
            assert (float(v) - lo) * 1024.0 == ext * k, "exact in double as well"
    on = table[table[:, 3] == 0]
    assert on.shape[0] == 3 * 1023
    tri = scene.positions[scene.indices[on[:, 0]]]  # [n, 3 vertices, 3 axes]
    flat = tri[np.arange(on.shape[0]), :, on[:, 1]]
    want = np.array([E.cell_boundary(a, k) for _, a, k, _ in on], np.float32)
    assert (flat == want[:, None]).all(), "flat on its axis: the tight-box midpoint is the boundary itself"


def test_cell_edges_codes_step_exactly_at_the_boundaries(cells):
    """On the boundary k the axis code is k, one float32 above it k, one float32 below it k - 1: all 3 x 1023.

    One boundary cannot do the last as stated: x boundary 512 is 0.0, whose float32 neighbours are +-2^-149, and the
    definition's own rounded double subtraction mid - slo = -2^-149 + 1.5 is 1.5: the code is 512 by csrc/lbvh.h, not
    511.  The triangle stays in the scene (the kernels must agree with the host on it); its code is asserted to be what
    the arithmetic says, and a further triangle at -2^-52, the float32 nearest below 0 that 1.5 + v resolves in double,
    carries the k - 1 statement for that boundary."""
    _, table, code = cells
    q = E.axis_codes(code[table[:, 0]], 0), E.axis_codes(code[table[:, 0]], 1), E.axis_codes(code[table[:, 0]], 2)
    got = np.choose(table[:, 1], q)
    k, which = table[:, 2], table[:, 3]
    absorbed = (table[:, 1] == 0) & (k == 512) & (which == -1)
    assert absorbed.sum() == 1 and float(np.float64(1.5) + np.float64(-2.0 ** -149)) == 1.5
    assert float(np.float64(1.5) + np.float64(E.CELL_X0_RESOLVED)) < 1.5 == float(np.float64(1.5) - 2.0 ** -53)
    want = np.where(which >= 0, k, k - 1)
    want[absorbed] = 512
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, table[bad[:8]], got[bad[:8]])
    for w in (-1, 0, 1):
        assert (which == w).sum() == 3 * 1023
    assert (which == -2).sum() == 1 and got[which == -2][0] == 511
    # every code 1 .. 1023 is reached from both sides on every axis
    for axis in range(3):
        sel = table[:, 1] == axis
        assert set(got[sel & (which == 0)]) == set(range(1, 1024)) and set(got[sel & (which == -1)]) >= set(range(0, 511))


def test_cell_edges_host_builder_matches_the_checker(cells):
    _lbvh_equals_checker(cells[0])


# ---------------------------------------------------------------------------------------------- small counts

@pytest.mark.parametrize("nt", E.SMALL_COUNTS)
def test_small_count_host_builder_and_refit_match_the_checkers(nt):
    from rsd.frame import host_bvh, host_bvh_refit
    scene = E.soup(nt)
    assert scene.indices.shape[0] == nt and scene.indices[1, 0] == scene.indices[0, 0], "a shared vertex"
    bvh, off = _lbvh_equals_checker(scene)
    w, nn, nrec = layout(bvh, off)
    assert nrec == nt
    ref, cnt = w[24:28], w[28:32]
    if nt <= 4:  # the leaf root the host-side root[] copy writes, with cnt > 1
        assert nn == 1 and list(cnt) == [nt, 0, 0, 0] and list(ref) == [0, EMPTY, EMPTY, EMPTY]
    else:
        assert nn >= 1 and ((cnt > 0) | (ref != EMPTY)).sum() >= 2
    if nt in (17, 21):  # more than 8 triangles: a root half exceeds 4 and splits again
        assert ((cnt > 0) | (ref != EMPTY)).sum() in (3, 4)
    if nt in (6, 9):
        assert nn == 1 or ((cnt == 0) & (ref != EMPTY)).any()
    # the jittered refit of both trees (the SAH tree of the upload, the LBVH of a rebuild)
    p1 = E.jitter(scene)
    _lbvh_equals_checker(scene, p1)
    for tree, toff in (host_bvh(scene), (bvh, off)):
        out = host_bvh_refit(tree, toff, scene.indices, p1)
        assert np.array_equal(_u32(out), expected_refit(tree, toff, scene.indices, p1))
        assert not np.array_equal(_u32(out), _u32(tree))


def test_small_counts_cross_the_wave_and_the_block():
    ni = [nt - 1 for nt in E.SMALL_COUNTS]
    assert {63, 64, 65} <= set(ni) and {255, 256, 257} <= set(ni), "csrc/lbvh.hip: waves of 64 lanes, kLbvhBlock = 256"


# ---------------------------------------------------------------------------------------------- soup_176k

def test_soup_176k_box_is_defined_past_the_launch_cap():
    scene = E.soup_176k()
    nt = scene.indices.shape[0]
    assert nt == E.BIG_NT == 176_000
    # scene_box_kernel (csrc/lbvh.hip) is capped at 2048 blocks of 256 lanes, one index component per lane and trip
    assert 3 * nt > 2048 * 256 == E.BOX_CAP
    comps, at = E.box_defining_components(scene)
    assert at[comps].any(axis=0).all() and comps.size == 6, "one component per extreme of the box"
    assert comps.min() >= 0.9 * 3 * nt, "in the last tenth of the index buffer"
    assert comps.min() >= E.BOX_CAP, "past the cap: lanes read them on their second trip through the loop only"
    # without them the box is another one: a loop that stops after one trip changes the codes
    first = scene.positions[scene.indices.reshape(-1)[:E.BOX_CAP]]
    full = scene.positions[scene.indices.reshape(-1)]
    assert (first.min(axis=0) > full.min(axis=0)).all() and (first.max(axis=0) < full.max(axis=0)).all()


def test_soup_176k_subsample_host_builder_matches_the_checker():
    """The numpy checker's recursion is not run on 176 000 triangles: a 1/16 subsample of the same generator, the six
    box-defining triangles included, pins the host builder that the GPU test of the whole scene compares with."""
    sub = E.soup_176k(every=16)
    assert sub.indices.shape[0] == (E.BIG_NT - 6 + 15) // 16 + 6
    full = E.soup_176k()
    assert np.array_equal(sub.positions[-18:], full.positions[-18:]) and np.array_equal(sub.positions[:3], full.positions[:3])
    _lbvh_equals_checker(sub)


# ---------------------------------------------------------------------------------------------- float classes

def _reaches_its_edge(base, cls, scene, p):
    used = p[np.unique(scene.indices)]
    mag = np.abs(used[used != 0])
    if cls == "denormal_mixed_sign":
        assert (mag < TINY).any() and (used < 0).any() and (used > 0).any()
        assert (_u32(p) == 0x80000000).any() and (_u32(p) == 0).any(), "zeros of both signs"
    elif cls == "huge":
        assert np.isfinite(p).all() and mag.max() > 1e37
        if base == "soup_400":  # the grid's coordinates are 0 .. 4: its extent stays below FLT_MAX
            ext = used.max(axis=0).astype(np.float64) - used.min(axis=0).astype(np.float64)
            assert (ext > FLT_MAX).all() and np.isfinite(ext).all(), "the extent overflows float32, not double"
            with np.errstate(over="ignore"):
                assert np.isinf(used.max(axis=0) - used.min(axis=0)).all()
    elif cls == "one_infinite":
        assert np.isposinf(used).sum() == 1 and not np.isnan(p).any()
    elif cls == "far_outside":
        assert np.abs(used).max() > 1000 and np.isfinite(p).all()
    elif cls == "collapsed":
        assert (p[scene.indices[0]] == p[scene.indices[0][0]]).all()
    elif cls == "unreferenced_outliers":
        nv = p.shape[0]
        assert scene.indices.max() < nv - E.OUTLIERS, "no triangle names them, and they are last in the buffer"
        assert p[-3, 0] == np.float32(1e30) and p[-2, 0] == np.float32(-1e30) and np.isnan(p[-1]).all()
        assert np.isfinite(used).all()


@pytest.mark.parametrize("cls", E.FLOAT_CLASSES)
@pytest.mark.parametrize("base", E.FLOAT_BASES)
def test_float_class_reaches_its_edge_and_the_host_matches_the_checkers(base, cls):
    from rsd.frame import host_bvh, host_bvh_lbvh, host_bvh_refit
    scene, p = E.float_class(base, cls)
    assert p.dtype == np.float32 and p.shape == scene.positions.shape and np.isfinite(scene.positions).all()
    _reaches_its_edge(base, cls, scene, p)
    built, off = host_bvh(scene)
    out = host_bvh_refit(built, off, scene.indices, p)
    assert np.array_equal(_u32(out), expected_refit(built, off, scene.indices, p)), "refit of the upload's tree"
    tree, toff = _lbvh_equals_checker(scene, p)
    back = host_bvh_refit(tree, toff, scene.indices, scene.positions)
    assert np.array_equal(_u32(back), expected_refit(tree, toff, scene.indices, scene.positions)), "and back"
    if cls == "unreferenced_outliers":
        bare = dataclasses.replace(scene, positions=np.ascontiguousarray(p[:-E.OUTLIERS]))
        alone, aoff = host_bvh_lbvh(bare)
        assert aoff == toff and np.array_equal(_u32(alone), _u32(tree)), "vertices no triangle names change no byte"
    if cls == "one_infinite":  # that axis of the triangle quantises to 0: the code still exists
        axis1 = E.axis_codes(lbvh_checker.codes(p, scene.indices), 1)
        assert axis1.max() == 0, "an infinite scene box: every code of that axis is 0"


@pytest.mark.parametrize("cls", E.FINITE_CLASSES)
@pytest.mark.parametrize("base", E.FLOAT_BASES)
def test_finite_classes_build_as_an_upload_would(base, cls):
    """The GPU test uploads the finite classes fresh, which runs the SAH builder (rsd_bvh_build) at those positions.
    Its bin index was (int)((c - lo) * scale) with scale = 32 / extent: infinite for a denormal extent, 0 for one that
    overflows float32, so the product was infinite or NaN, its conversion came out negative and the builder wrote in
    front of its bins (a crash on denormal_mixed_sign and on the huge soup).  The tree must be one rsd_bvh_refit
    accepts and leaves alone, with every primitive in one record."""
    from rsd.frame import host_bvh, host_bvh_refit
    scene, p = E.float_class(base, cls)
    at_p = dataclasses.replace(scene, positions=p)
    bvh, off = host_bvh(at_p)
    w, nn, nrec = layout(bvh, off)
    nt = scene.indices.shape[0]
    assert nrec == nt and nn >= 1
    prim = w[4 * off:4 * off + 12 * nt].reshape(nt, 3, 4)[:, 0, 3]
    assert np.array_equal(np.sort(prim), np.arange(nt))
    assert w[:32 * nn].reshape(nn, 8, 4)[:, 7, :].max() <= 4
    assert np.array_equal(_u32(host_bvh_refit(bvh, off, scene.indices, p)), _u32(bvh))
    assert np.array_equal(expected_refit(bvh, off, scene.indices, p), _u32(bvh))


def test_a_referenced_nan_gives_a_tree_the_refit_accepts():
    """A NaN coordinate of a vertex a triangle names.  The numpy checkers are no reference here: float min / max
    propagate a NaN, the shared headers (csrc/bvh_refit.h) order it by its integer key, above +inf.  So only this is
    asserted on the CPU: rsd_bvh_refit accepts the host builder's tree (refit_topology) and is the identity on it, and
    the NaN is where it was meant to be.  tests/test_gpu_dynamic_edges.py compares the kernels with the host bytes."""
    from rsd.frame import host_bvh, host_bvh_lbvh, host_bvh_refit
    scene, p = E.referenced_nan()
    assert np.isnan(p).sum() == 1 and np.isnan(p[np.unique(scene.indices)]).sum() == 1
    assert (_u32(p)[np.isnan(p)] == 0x7FC00000).all()
    tree, off = host_bvh_lbvh(dataclasses.replace(scene, positions=p))
    _, nn, nrec = layout(tree, off)
    assert nrec == scene.indices.shape[0] and nn > 4
    assert np.array_equal(_u32(host_bvh_refit(tree, off, scene.indices, p)), _u32(tree))
    built, boff = host_bvh(scene)
    out = host_bvh_refit(built, boff, scene.indices, p)
    assert np.isnan(out).any() and not np.array_equal(_u32(out), _u32(built))


# ---------------------------------------------------------------------------------------------- update_subset

def test_subset_grid_puts_the_parent_table_right_after_the_positions():
    """include/rsd.h: an id >= vertex_count moves nothing.  With 12 * nv a multiple of 256 the refit's parent table
    follows the positions without a gap (csrc/rsd_internal.h dyn_layout aligns to 256), so a store through id nv or
    nv + 1 would land in the parent words of nodes 0 .. 5 -- inside the allocation -- and show as wrong boxes."""
    from rsd.frame import host_bvh
    scene = E.subset_grid()
    nv = scene.positions.shape[0]
    assert nv == 320 and nv % 64 == 0 and (12 * nv) % 256 == 0 and nv > 257
    assert np.array_equal(np.unique(scene.indices), np.arange(nv)), "every vertex is named: export_positions sees all"
    _, off = host_bvh(scene)
    assert off // 8 >= 6, "six parent words exist behind the positions"


# ---------------------------------------------------------------------------------------------- motion snapshot

@pytest.fixture(scope="module")
def mvref(oracle, tmp_path_factory):
    return oracle, MV.build(oracle, tmp_path_factory.mktemp("mvec_ref"))


@pytest.mark.parametrize("nv", E.SNAPSHOT_NV)
def test_snapshot_grid_shows_its_last_vertex(mvref, nv):
    """3 * nv mod 4 is 0, 3, 2, 1 (and 1 for 1027): the dword tail of motion_snapshot_kernel's copy.  The expected
    motion vectors P1 -> P2 have a non-zero pixel owned by a triangle that names the last vertex, and they differ from
    the vectors of a snapshot whose tail dwords were never copied (those still hold the upload's numbers)."""
    O, lib = mvref
    scene = E.snapshot_grid(nv)
    assert (3 * nv) % 4 == {20: 0, 21: 3, 22: 2, 23: 1, 1027: 1}[nv]
    if nv == 1027:
        assert 3 * nv // 4 > 256 * 3, "more vector lanes than one block, then the tail"
    p1, p2 = E.snapshot_motion(scene)
    size = MV.SIZES[0]
    cam = MV.camera(scene, size)
    want = MV.run(O, lib, scene, p2, p1, cam, cam, size, 0)
    hit = want["prim"] != MV.MISS
    owner = np.zeros(hit.shape, bool)
    owner[hit] = (scene.indices[want["prim"][hit]] == nv - 1).any(axis=-1)
    assert owner.any() and MV.bits(want["mvec"])[owner].any(), "the last vertex moves pixels"
    if nv < 100:  # the 32 x 32 grid has more triangles than some of them can own pixel centres
        assert set(np.unique(scene.indices[want["prim"][hit]])) == set(range(nv)), "every vertex is in a visible triangle"
    tail = (3 * nv) % 4
    if tail:
        stale = p1.copy()
        stale.reshape(-1)[-tail:] = scene.positions.reshape(-1)[-tail:]
        assert (_u32(stale) != _u32(p1)).sum() == tail
        other = MV.run(O, lib, scene, p2, stale, cam, cam, size, 0)
        assert (MV.bits(other["mvec"]) != MV.bits(want["mvec"]))[owner].any(), "a tail left uncopied shows"
