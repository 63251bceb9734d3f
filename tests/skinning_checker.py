"""An independent statement of rsd_scene_update_pose's arithmetic (include/rsd.h, DESIGN.md 4 "Animated scenes") in
numpy float32.  numpy never fuses a multiply with an add, so each line below is one rounded operation per element,
in the order the header gives:

    B[e]   = ((M[i0][e] * w0 + M[i1][e] * w1) + M[i2][e] * w2) + M[i3][e] * w3      for the 12 elements e
    out[r] = ((B[r][0] * x + B[r][1] * y) + B[r][2] * z) + B[r][3]                  for the rows r = 0, 1, 2

All four slots are evaluated whatever their weights, nothing is normalised, and a vertex outside the rig keeps its
position.  Written as a loop over the four slots and the three rows on purpose: it shares no code with rsd.animation."""
import numpy as np

F = np.float32


def rest_positions(positions, rig):
    """The positions the matrices act on: the rig's own rest positions, else `positions` at its vertices."""
    if getattr(rig, "rest", None) is not None:
        return np.asarray(rig.rest, F).reshape(-1, 3)
    return np.asarray(positions, F).reshape(-1, 3)[np.asarray(rig.vertex_ids, np.int64)]


def posed(positions, rig, matrices, rest=None):
    """The full position array [nv, 3] after a pose: `positions` (what the scene holds before it) with the rig's
    vertices replaced.  rest: the rest positions of the rig's vertices if they are not rest_positions(positions, rig)."""
    out = np.array(positions, F).reshape(-1, 3).copy()
    if rig.vertex_ids.size == 0:
        return out
    M = np.asarray(matrices, F).reshape(-1, 3, 4)
    assert M.shape[0] == rig.matrix_count
    ids = np.asarray(rig.matrix_ids, np.int64).reshape(-1, 4)
    w = np.asarray(rig.weights, F).reshape(-1, 4)
    r = rest_positions(positions, rig) if rest is None else np.asarray(rest, F).reshape(-1, 3)
    B = np.empty((ids.shape[0], 3, 4), F)
    for row in range(3):
        for col in range(4):
            t0 = M[ids[:, 0], row, col] * w[:, 0]
            t1 = M[ids[:, 1], row, col] * w[:, 1]
            t2 = M[ids[:, 2], row, col] * w[:, 2]
            t3 = M[ids[:, 3], row, col] * w[:, 3]
            s = t0 + t1
            s = s + t2
            B[:, row, col] = s + t3
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    v = np.asarray(rig.vertex_ids, np.int64)
    for row in range(3):
        a = B[:, row, 0] * x
        b = B[:, row, 1] * y
        c = B[:, row, 2] * z
        s = a + b
        s = s + c
        out[v, row] = s + B[:, row, 3]
    assert out.dtype == F
    return out


def random_matrices(rng, count, translation=1.0):
    """`count` rotation x scale + translation matrices as float32 [count, 12] (rows, translation in column 3)."""
    out = np.zeros((count, 3, 4), np.float64)
    for k in range(count):
        q = rng.standard_normal(4)
        q /= np.linalg.norm(q)
        x, y, z, w = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        out[k, :, :3] = R * rng.uniform(0.6, 1.5, 3)[None, :]
        out[k, :, 3] = translation * rng.uniform(-1.0, 1.0, 3)
    return out.reshape(count, 12).astype(F)


def identity_matrices(count):
    return np.tile(np.eye(4, dtype=F)[:3].reshape(12), (count, 1))
