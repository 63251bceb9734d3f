"""An independent statement of what a BVH refit must produce (tests/test_bvh_refit.py, tests/test_gpu_scene_update.py).

`expected_refit` walks an exported BVH (rsd_bvh_build / rsd_scene_export_bvh bytes) in numpy: it rewrites each
record's nine position floats from the index buffer and the new positions, and recomputes for every child slot the
tight min / max over all record vertices under that child, moved two floats outward with np.nextafter.  Nothing of
librsd's refit is used: float min / max and nextafter here, integer keys and bit steps there.  Everything else -- ref,
cnt, prim, flags, the zeros of empty slots, the pad -- is copied, so equality with the result also says those words
were left alone."""
import sys

import numpy as np

EMPTY = 0xFFFFFFFF


def layout(bvh, tri_offset):
    """(words, node count, record count) of BVH bytes given as a float32 / uint32 array."""
    w = np.ascontiguousarray(bvh).view(np.uint32)
    nn = tri_offset // 8
    rest = w.size - 4 * tri_offset - 48
    assert tri_offset % 8 == 0 and rest >= 0 and rest % 12 == 0, (w.size, tri_offset)
    return w, nn, rest // 12


def _pad(lo, hi):
    f = np.float32
    lo = np.nextafter(np.nextafter(lo, f(-np.inf)), f(-np.inf))
    hi = np.nextafter(np.nextafter(hi, f(np.inf)), f(np.inf))
    return lo, hi


def expected_refit(bvh, tri_offset, indices, positions):
    w, nn, nrec = layout(bvh, tri_offset)
    out = w.copy()
    f = out.view(np.float32)
    ind = np.asarray(indices, np.uint32).reshape(-1, 3)
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    recs = f[4 * tri_offset:4 * tri_offset + 12 * nrec].reshape(nrec, 3, 4)
    prim = out[4 * tri_offset:4 * tri_offset + 12 * nrec].reshape(nrec, 3, 4)[:, 0, 3].copy()
    assert nrec == ind.shape[0] and np.array_equal(np.sort(prim), np.arange(nrec)), "one record per triangle"
    recs[:, :, :3] = pos[ind[prim]]
    nodes_u = out[:32 * nn].reshape(nn, 8, 4)
    nodes_f = f[:32 * nn].reshape(nn, 8, 4)
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 1000))

    def tight(n):
        los, his = [], []
        for i in range(4):
            ref, cnt = int(nodes_u[n, 6, i]), int(nodes_u[n, 7, i])
            if cnt:
                v = recs[ref:ref + cnt, :, :3].reshape(-1, 3)
                lo, hi = v.min(axis=0), v.max(axis=0)
            elif ref != EMPTY:
                lo, hi = tight(ref)
            else:
                continue
            plo, phi = _pad(lo, hi)
            nodes_f[n, 0:6:2, i] = plo
            nodes_f[n, 1:6:2, i] = phi
            los.append(lo)
            his.append(hi)
        return np.min(los, axis=0), np.max(his, axis=0)

    try:
        if nrec:
            tight(0)
    finally:
        sys.setrecursionlimit(limit)
    return out


def topology_words(bvh, tri_offset):
    """The words a refit must never write: every ref and cnt, every record's fourth words (prim, flags, 0), the pad."""
    w, nn, nrec = layout(bvh, tri_offset)
    nodes = w[:32 * nn].reshape(nn, 8, 4)[:, 6:, :].ravel()
    recs = w[4 * tri_offset:4 * tri_offset + 12 * nrec].reshape(nrec, 3, 4)[:, :, 3].ravel()
    return np.concatenate([nodes, recs, w[4 * tri_offset + 12 * nrec:]])
