"""An independent statement of rsd_scene_update_pose_morph's arithmetic (include/rsd.h, DESIGN.md 4 "glTF and morph
targets") in numpy float32, on top of tests/skinning_checker.py.  For rig vertex i, from p = rest[i], for each entry e
of offsets[i] .. offsets[i + 1] - 1 in ascending order and each component c:

    p.c = p.c + (w[id_e] * delta_e.c)

the product rounded to float32, then the sum; every entry is evaluated, a weight of 0 included; then
skinning_checker.posed runs on p in place of the rest position.  A vertex without entries gets posed()'s bits.
Written as a scalar loop over vertices and entries on purpose: it shares no code with rsd.animation.

table_from_targets restates the rule that makes a table from morph targets: target k of vertex v becomes an entry
only if at least one component of its delta is not +-0."""
import numpy as np

import skinning_checker

F = np.float32


def morphed_rest(rest, offsets, weight_ids, deltas, weights):
    """float32 [count, 3]: the rest positions with the morph sum applied."""
    p = np.array(rest, F).reshape(-1, 3).copy()
    off = np.asarray(offsets, np.int64).reshape(-1)
    ids = np.asarray(weight_ids, np.int64).reshape(-1)
    d = np.asarray(deltas, F).reshape(-1, 3)
    w = np.asarray(weights, F).reshape(-1)
    assert off.size == p.shape[0] + 1 and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == ids.size
    for i in range(p.shape[0]):
        for e in range(off[i], off[i + 1]):
            wk = w[ids[e]]
            for c in range(3):
                prod = F(wk * d[e, c])
                p[i, c] = F(p[i, c] + prod)
    assert p.dtype == F
    return p


def posed(positions, rig, matrices, offsets, weight_ids, deltas, weights, rest=None):
    """The full position array [nv, 3] after rsd_scene_update_pose_morph."""
    r = skinning_checker.rest_positions(positions, rig) if rest is None else np.asarray(rest, F).reshape(-1, 3)
    return skinning_checker.posed(positions, rig, matrices, rest=morphed_rest(r, offsets, weight_ids, deltas, weights))


def export_positions(gs, indices):
    """The positions the device's triangle records hold (rsd.frame.GpuScene.export_bvh), float32 [vertex_count, 3]:
    the record of primitive p holds the positions of indices[p] as the last update left them, bit for bit.  A vertex no
    triangle names cannot be read and comes back as NaN."""
    bvh, off = gs.export_bvh()
    ind = np.asarray(indices, np.int64).reshape(-1, 3)
    rec = bvh.view(np.uint32)[4 * off:][:12 * ind.shape[0]].reshape(-1, 3, 4)
    out = np.full((gs.vertex_count, 3), np.nan, F)
    out.view(np.uint32)[ind[rec[:, 0, 3]].reshape(-1)] = rec[:, :, :3].reshape(-1, 3)
    return out


def table_from_targets(targets, first_weight=0):
    """targets: float32 [k, n, 3] -- (offsets [n + 1], weight_ids, deltas [entries, 3]) of n vertices, the entries of a
    vertex in target order, a target whose delta is +-0 in every component left out."""
    t = np.asarray(targets, F)
    offsets, ids, deltas = [0], [], []
    for v in range(t.shape[1]):
        for k in range(t.shape[0]):
            if any(float(x) != 0.0 for x in t[k, v]):
                ids.append(first_weight + k)
                deltas.append(t[k, v])
        offsets.append(len(ids))
    return (np.array(offsets, np.uint32), np.array(ids, np.uint32),
            np.array(deltas, F).reshape(-1, 3))
