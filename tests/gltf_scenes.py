"""glTF documents of the importer's tests (tests/gltf_writer.py), shared by the CPU and the GPU tests.

cylinder(): a two-joint skinned cylinder of 2 x 8 vertices with a cap and two morph targets, animated, above a static
floor, with a camera node.  Test infrastructure only."""
import numpy as np

import gltf_writer as G

RING = 8
CYL_TIMES = (0.0, 0.4, 1.1)   # the times the tests pose at: a key, between keys, past the last weight key


def quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([a * np.sin(0.5 * angle), [np.cos(0.5 * angle)]])


def cylinder(mesh_translation=(0.0, 0.0, 0.0), camera=True):
    """Nodes: 0 joint A (root, translation animated LINEAR), 1 joint B (child of A at y = 0.5, rotation animated
    LINEAR), 2 the skinned mesh node (its own translation must not matter; node.weights override mesh.weights), 3 the
    static floor, 4 the camera.  Returns (writer, info)."""
    w = G.Writer()
    ang = 2.0 * np.pi * np.arange(RING) / RING
    ring = np.stack([0.5 * np.cos(ang), np.zeros(RING), 0.5 * np.sin(ang)], 1)
    pos = np.concatenate([ring, ring + [0.0, 1.0, 0.0]]).astype(np.float32)
    tri = []
    for k in range(RING):
        a, b, c, d = k, (k + 1) % RING, RING + (k + 1) % RING, RING + k
        tri += [[a, c, b], [a, d, c]]
    tri += [[RING, RING + k + 1, RING + k] for k in range(1, RING - 1)]  # the cap, facing +y
    joints = np.zeros((2 * RING, 4), np.uint8)
    joints[:, 1] = 1
    weights = np.zeros((2 * RING, 4), np.float32)
    weights[:RING, 0] = 1.0
    weights[RING:, :2] = (0.25, 0.75)
    # target 0 lifts and widens the cap ring; target 1 shears every other vertex in x (the rest: exactly 0)
    t0 = np.zeros_like(pos)
    t0[RING:] = pos[RING:] * [0.5, 0.0, 0.5] + [0.0, 0.25, 0.0]
    t1 = np.zeros_like(pos)
    t1[1::2, 0] = 0.125
    t1[3, 0] = -0.0  # a -0 delta is no entry either
    ibm = np.tile(np.eye(4), (2, 1, 1))
    ibm[1, 1, 3] = -0.5  # inverse of joint B's rest global (translation y = 0.5)
    prim = {"attributes": {"POSITION": w.accessor(pos), "JOINTS_0": w.accessor(joints, G.UBYTE),
                           "WEIGHTS_0": w.accessor(weights)},
            "indices": w.accessor(np.asarray(tri).reshape(-1), G.UBYTE),
            "targets": [{"POSITION": w.accessor(t0)}, {"POSITION": w.accessor(t1)}]}
    mesh = w.add("meshes", {"name": "cylinder", "primitives": [prim], "weights": [0.5, 0.25]})
    floor = np.array([[-2, -0.5, -2], [2, -0.5, -2], [2, -0.5, 2], [-2, -0.5, 2]], np.float32)
    fmesh = w.add("meshes", {"name": "floor", "primitives": [
        {"attributes": {"POSITION": w.accessor(floor)}, "indices": w.accessor(np.array([0, 2, 1, 0, 3, 2]), G.USHORT)}]})
    skin = w.add("skins", {"joints": [0, 1], "inverseBindMatrices": w.accessor(
        ibm.transpose(0, 2, 1).reshape(2, 16), atype="MAT4")})
    w.add("nodes", G.trs_node(translation=[0.1, 0.0, 0.0], children=[1], name="jointA"))
    w.add("nodes", G.trs_node(translation=[0.0, 0.5, 0.0], children=[], name="jointB"))
    w.add("nodes", G.trs_node(translation=mesh_translation, mesh=mesh, skin=skin, weights=[0.75, 0.25], name="body"))
    w.add("nodes", G.trs_node(mesh=fmesh, name="floor"))
    roots = [0, 2, 3]
    if camera:
        cam = w.add("cameras", {"type": "perspective", "perspective": {"yfov": 0.8, "znear": 0.1, "zfar": 100.0}})
        w.add("nodes", G.trs_node(translation=[0.2, 1.6, 2.6], rotation=quat([1, 0, 0], -0.45), camera=cam,
                                  name="camera"))
        roots.append(4)
    w.doc["scenes"] = [{"nodes": roots}]
    w.doc["scene"] = 0
    info = dict(
        a_times=[0.0, 1.0], a_values=[[0.1, 0.0, 0.0], [0.3, 0.2, -0.1]],
        b_times=[0.0, 0.5, 1.0], b_values=[quat([0, 0, 1], 0.0), quat([0, 0, 1], 0.6), quat([1, 0, 1], -0.4)],
        w_times=[0.0, 0.5, 1.0], w_values=[[0.75, 0.25], [0.0, 1.0], [1.0, -0.5]],
        ibm=ibm, positions=pos, triangles=np.asarray(tri), joints=joints, weights=weights, targets=np.stack([t0, t1]),
        cylinder_vertices=2 * RING, floor_vertices=4)
    G.add_animation(w, [(0, "translation", info["a_times"], info["a_values"], "LINEAR"),
                        (1, "rotation", info["b_times"], info["b_values"], "LINEAR")], "bend")
    G.add_animation(w, [(2, "weights", info["w_times"], info["w_values"], "LINEAR")], "shape")
    return w, info
