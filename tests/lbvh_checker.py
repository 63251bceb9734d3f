"""An independent statement of the tree rsd_bvh_build_lbvh / rsd_scene_rebuild_bvh must produce (DESIGN.md 4
"Rebuilding topology on the GPU"; tests/test_lbvh.py, tests/test_gpu_lbvh.py).

`expected_lbvh` restates the definition top-down in numpy / Python: float min / max for the boxes, float64 arithmetic
for the codes, a bit-by-bit interleave, numpy's sort, and a recursion that splits a range of sorted keys with a binary
search for the first key whose highest differing bit is set.  librsd's builder works bottom-up instead (one Karras node
per internal node, depths up a parent chain, numbers from a second sort) on integer keys; nothing of csrc/lbvh.h is used
here.  Boxes and record positions come from tests/bvh_refit_checker.py's recomputation."""
import numpy as np

from bvh_refit_checker import EMPTY, expected_refit

LEAF = 4


def codes(positions, indices):
    """30-bit Morton codes per triangle: per axis the midpoint of the triangle's tight box, quantised to 10 bits inside
    the tight box of all referenced vertices; x in the highest bit of each triple."""
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    ind = np.asarray(indices, np.uint32).reshape(-1, 3)
    tri = pos[ind]                                # [nt, 3 vertices, 3 axes]
    lo, hi = tri.min(axis=1), tri.max(axis=1)     # float32, exact
    slo, shi = lo.min(axis=0), hi.max(axis=0)
    with np.errstate(all="ignore"):
        ext = shi.astype(np.float64) - slo.astype(np.float64)
        mid = (lo.astype(np.float64) + hi.astype(np.float64)) * 0.5
        q = (mid - slo.astype(np.float64)) / ext * 1024.0
    ok = np.isfinite(lo) & np.isfinite(hi) & np.isfinite(slo)[None] & np.isfinite(shi)[None] & (ext > 0.0)[None]
    q = np.where(ok & (q >= 0.0), q, 0.0)         # NaN compares false
    q = np.minimum(q, 1023.0).astype(np.uint64)   # truncation
    code = np.zeros(ind.shape[0], np.uint64)
    for bit in range(10):
        for axis in range(3):
            code |= ((q[:, axis] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + 2 - axis)
    return code


def sorted_keys(positions, indices):
    nt = np.asarray(indices).reshape(-1, 3).shape[0]
    keys = (codes(positions, indices) << np.uint64(32)) | np.arange(nt, dtype=np.uint64)
    return np.sort(keys)


def _split(keys, a, b):
    """Last position of the left part of [a, b]: the keys whose highest bit in which keys[a] and keys[b] differ is 0."""
    top = (int(keys[a]) ^ int(keys[b])).bit_length() - 1
    assert top >= 0, "keys are distinct"
    boundary = ((int(keys[a]) >> top) | 1) << top  # the smallest key of the range's prefix with that bit set
    return a + int(np.searchsorted(keys[a:b + 1], np.uint64(boundary), side="left")) - 1


def tree(keys):
    """The wide nodes of the definition as a list of (level, first position, [child ranges (a, b)]) sorted by
    (level, first position) -- the node numbering -- for more than LEAF keys."""
    out = []

    def wide(a, b, level):
        kids = []
        s = _split(keys, a, b)
        for ha, hb in ((a, s), (s + 1, b)):
            if hb - ha + 1 > LEAF:
                t = _split(keys, ha, hb)
                kids += [(ha, t), (t + 1, hb)]
            else:
                kids.append((ha, hb))
        out.append((level, a, kids))
        for ca, cb in kids:
            if cb - ca + 1 > LEAF:
                wide(ca, cb, level + 1)

    wide(0, len(keys) - 1, 0)
    out.sort(key=lambda n: (n[0], n[1]))
    return out


def depth_bound(nt):
    """Wide nodes on a path at most: (30 + ceil(log2 nt)) // 2 + 1."""
    return (30 + max(0, int(nt) - 1).bit_length()) // 2 + 1


def expected_lbvh(positions, indices, flags=None):
    """(uint32 words of the whole BVH, tri_offset in float4 units, wide depth)."""
    ind = np.asarray(indices, np.uint32).reshape(-1, 3)
    nt = ind.shape[0]
    keys = sorted_keys(positions, ind)
    prim = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    if nt > LEAF:
        nodes = tree(keys)
        number = {(lv, a): n for n, (lv, a, _) in enumerate(nodes)}
    else:
        nodes = [(0, 0, [(0, nt - 1)] if nt else [])]
        number = {}
    nn = len(nodes)
    w = np.zeros(32 * nn + 12 * nt + 48, np.uint32)
    nd = w[:32 * nn].reshape(nn, 8, 4)
    nd[:, 6, :] = EMPTY
    for n, (lv, _, kids) in enumerate(nodes):
        assert 1 <= len(kids) <= 4 or nt == 0
        for i, (a, b) in enumerate(kids):
            if b - a + 1 > LEAF:
                nd[n, 6, i] = number[(lv + 1, a)]
            else:
                nd[n, 6, i], nd[n, 7, i] = a, b - a + 1
    recs = w[32 * nn:32 * nn + 12 * nt].reshape(nt, 3, 4)
    recs[:, 0, 3] = prim
    recs[:, 1, 3] = 0 if flags is None else np.asarray(flags, np.uint32)[prim]
    out = expected_refit(w, 8 * nn, ind, positions)
    return out, 8 * nn, nodes[-1][0] + 1
