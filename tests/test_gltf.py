"""CPU: the glTF 2.0 importer (rsd/gltf.py) on documents written by tests/gltf_writer.py: containers, accessors,
strips and fans, node matrices, materials, the camera, animation samplers against closed forms in float64, skins against
an independent float64 evaluation, and the routing from rsd.pyscene.  Morph targets: tests/test_morph.py."""
import math

import numpy as np
import pytest

import gltf_scenes
import gltf_writer as G
from gltf_scenes import quat

F = np.float32


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _quad():
    pos = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0.5], [0, 1, 0.25], [2, 2, 2]], F)
    tri = np.array([[0, 1, 2], [0, 2, 3], [2, 1, 4]])
    return pos, tri


def _one_mesh(w, prim, node=None, **mesh_kw):
    m = w.add("meshes", dict(primitives=[prim], **mesh_kw))
    w.add("nodes", dict(node or {}, mesh=m))
    return w


def _trs(t=(0, 0, 0), q=(0, 0, 0, 1), s=(1, 1, 1)):
    """T * R * S in float64, written out here (not rsd.animation's)."""
    x, y, z, w = (float(v) for v in q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    M = np.eye(4)
    M[:3, :3] = R * np.asarray(s, np.float64)[None, :]
    M[:3, 3] = t
    return M


# ---------------------------------------------------------------------------------- containers and accessors

def test_three_containers_import_to_identical_arrays(tmp_path):
    from rsd.gltf import load_gltf
    w, _ = gltf_scenes.cylinder()
    scenes = [load_gltf(w.save(tmp_path / name, kind)) for kind, name in
              (("gltf", "a.gltf"), ("datauri", "b.gltf"), ("glb", "c.glb"))]
    assert (tmp_path / "a.bin").exists() and "data:" in (tmp_path / "b.gltf").read_text()
    assert (tmp_path / "c.glb").read_bytes()[:4] == b"glTF"
    a = scenes[0]
    assert a.positions.shape == (20, 3) and a.indices.shape == (24, 3) and a.rig.count == 16
    for b in scenes[1:]:
        for x, y in ((a.positions, b.positions), (a.indices, b.indices), (a.flags, b.flags),
                     (a.rig.vertex_ids, b.rig.vertex_ids), (a.rig.matrix_ids, b.rig.matrix_ids),
                     (a.rig.weights, b.rig.weights), (a.rig.rest, b.rig.rest), (a.rig.morph.offsets, b.rig.morph.offsets),
                     (a.rig.morph.weight_ids, b.rig.morph.weight_ids), (a.rig.morph.deltas, b.rig.morph.deltas),
                     (a.rig.matrices(0.4), b.rig.matrices(0.4))):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        assert a.camera == b.camera


def test_glb_container_rules(tmp_path):
    from rsd.gltf import GltfError, load_gltf
    w, _ = gltf_scenes.cylinder()
    data = bytearray(w.save(tmp_path / "c.glb", "glb").read_bytes())
    data[4:8] = (1).to_bytes(4, "little")
    (tmp_path / "v1.glb").write_bytes(data)
    with pytest.raises(GltfError, match="version 1"):
        load_gltf(tmp_path / "v1.glb")
    (tmp_path / "nojson.glb").write_bytes(b"glTF" + (2).to_bytes(4, "little") + (12).to_bytes(4, "little"))
    with pytest.raises(GltfError, match="JSON chunk"):
        load_gltf(tmp_path / "nojson.glb")
    # a GLB without a BIN chunk: a scene of nodes only
    e = G.Writer()
    e.add("nodes", {})
    assert load_gltf(e.save(tmp_path / "empty.glb", "glb")).positions.shape == (0, 3)


@pytest.mark.parametrize("component", [G.UBYTE, G.USHORT, G.UINT])
def test_index_component_types(tmp_path, component):
    from rsd.gltf import load_gltf
    pos, tri = _quad()
    w = G.Writer()
    _one_mesh(w, {"attributes": {"POSITION": w.accessor(pos, lead=6)},
                  "indices": w.accessor(tri.reshape(-1), component, lead=3, skip=4 * np.dtype(G.DTYPE[component]).itemsize)})
    s = load_gltf(w.save(tmp_path / "i.gltf"))
    assert np.array_equal(s.indices, tri) and s.indices.dtype == np.uint32
    assert _u32(s.positions).tobytes() == _u32(pos).tobytes()
    acc = w.doc["accessors"][1]
    assert acc["byteOffset"] > 0 and w.doc["bufferViews"][acc["bufferView"]]["byteOffset"] > 0


@pytest.mark.parametrize("component", [G.UBYTE, G.USHORT])
def test_normalised_weights_and_uvs(tmp_path, component):
    """c / max, evaluated in float64 and rounded once, for skin weights and texture coordinates."""
    from rsd.gltf import load_gltf_builder
    pos, tri = _quad()
    top = np.iinfo(np.dtype(G.DTYPE[component])).max
    wq = np.array([[top, 0, 0, 0], [top // 3, top - top // 3, 0, 0], [1, 2, 3, top - 6], [0, 0, 0, 0], [7, 0, top - 7, 0]])
    uvq = np.array([[0, 0], [top, 0], [top, top], [1, top // 2], [top // 7, 3]])
    w = G.Writer()
    for _ in range(2):
        w.add("nodes", {})
    skin = w.add("skins", {"joints": [0, 1]})
    att = {"POSITION": w.accessor(pos), "JOINTS_0": w.accessor(np.array([[0, 1, 0, 1]] * 5), G.USHORT),
           "WEIGHTS_0": w.accessor(wq / top, component, normalized=True),
           "TEXCOORD_0": w.accessor(uvq / top, component, normalized=True)}
    _one_mesh(w, {"attributes": att, "indices": w.accessor(tri.reshape(-1), G.UBYTE)}, node={"skin": skin})
    B = load_gltf_builder(w.save(tmp_path / "n.gltf"))
    m = B.meshes[0]
    assert m.weights.dtype == F and np.array_equal(m.weights, (wq.astype(np.float64) / top).astype(F))
    assert np.array_equal(m.texcoords, (uvq.astype(np.float64) / top).astype(F))
    assert m.joints.dtype == np.uint32 and np.array_equal(m.joints, [[0, 1, 0, 1]] * 5)
    rig = B.build().rig
    assert np.array_equal(rig.weights, m.weights), "weights are taken as stored, not renormalised"


def test_byte_stride_20_interleaved(tmp_path):
    from rsd.gltf import load_gltf_builder
    pos, tri = _quad()
    uv = np.array([[0.1, 0.2], [0.9, 0.2], [0.9, 0.8], [0.1, 0.8], [0.5, 0.5]], F)
    w = G.Writer()
    a_pos, a_uv = w.interleaved([pos, uv], stride=20, lead=8)
    assert w.doc["bufferViews"][0]["byteStride"] == 20 and w.doc["accessors"][a_uv]["byteOffset"] == 12
    _one_mesh(w, {"attributes": {"POSITION": a_pos, "TEXCOORD_0": a_uv}, "indices": w.accessor(tri.reshape(-1), G.UBYTE)})
    m = load_gltf_builder(w.save(tmp_path / "s.glb", "glb")).meshes[0]
    assert m.positions.tobytes() == pos.tobytes() and m.texcoords.tobytes() == uv.tobytes()


def test_strip_and_fan_of_five_vertices(tmp_path):
    """Specification 3.7.2.1: strip p_i = (v_i, v_(i+1+i%2), v_(i+2-i%2)); fan p_i = (v_(i+1), v_(i+2), v_0)."""
    from rsd.gltf import load_gltf_builder
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 2, 0]], F)
    order = [4, 2, 0, 1, 3]
    want = {5: ([[0, 1, 2], [1, 3, 2], [2, 3, 4]], [[4, 2, 0], [2, 1, 0], [0, 1, 3]]),
            6: ([[1, 2, 0], [2, 3, 0], [3, 4, 0]], [[2, 0, 4], [0, 1, 4], [1, 3, 4]])}
    w = G.Writer()
    p = w.accessor(pos)
    prims = []
    for mode in (5, 6):
        prims += [{"attributes": {"POSITION": p}, "mode": mode},
                  {"attributes": {"POSITION": p}, "mode": mode, "indices": w.accessor(np.array(order), G.UBYTE)}]
    prims += [{"attributes": {"POSITION": p}, "mode": m} for m in (0, 1, 3)]  # points and lines: skipped
    w.add("nodes", {"mesh": w.add("meshes", {"primitives": prims})})
    B = load_gltf_builder(w.save(tmp_path / "f.gltf"))
    assert len(B.meshes) == 4
    got = [m.indices.tolist() for m in B.meshes]
    assert got == [want[5][0], want[5][1], want[6][0], want[6][1]]


# ---------------------------------------------------------------------------------- nodes, materials, camera

def test_three_level_hierarchy_and_a_mesh_under_two_nodes(tmp_path):
    from rsd.gltf import load_gltf_builder
    pos, tri = _quad()
    M0 = _trs((1.5, -2.0, 0.25), quat([1, 2, 3], 0.7), (1.0, 2.0, 0.5))
    t1, q1, s1 = (0.3, 0.1, -4.0), quat([0, 1, 0], -1.1), (-1.0, 1.0, 1.0)  # mirrors: the winding flips
    M2 = _trs((0.0, 7.0, 0.0), quat([1, 0, 0], 0.2))
    w = G.Writer()
    mesh = w.add("meshes", {"primitives": [{"attributes": {"POSITION": w.accessor(pos)},
                                            "indices": w.accessor(tri.reshape(-1), G.UBYTE)}]})
    w.add("nodes", G.matrix_node(M0, children=[1], mesh=mesh))
    w.add("nodes", G.trs_node(t1, q1, s1, children=[2]))
    w.add("nodes", G.matrix_node(M2, mesh=mesh))
    w.add("nodes", {"name": "outside the scene", "mesh": mesh})
    w.doc["scenes"] = [{"nodes": [3]}, {"nodes": [0]}]
    w.doc["scene"] = 1
    B = load_gltf_builder(w.save(tmp_path / "h.gltf"))
    assert len(B.meshes) == 1 and [i for i, _ in B.instances] == [0, 0], "one mesh, one instance per node"
    world = M0 @ _trs(t1, q1, s1) @ M2
    assert np.array_equal(B.instances[0][1], M0.astype(F)) and np.array_equal(B.instances[1][1], world.astype(F))
    s = B.build()
    T = world.astype(F)
    assert s.positions[5:].tobytes() == (pos @ T[:3, :3].T + T[:3, 3]).astype(F).tobytes()
    assert np.allclose(s.positions[5:], pos.astype(np.float64) @ world[:3, :3].T + world[:3, 3], rtol=0, atol=2e-5)
    assert np.array_equal(s.indices[:3], tri) and np.array_equal(s.indices[3:], tri[:, [1, 0, 2]] + 5)
    assert s.rig is None
    assert len(load_gltf_builder(tmp_path / "h.gltf", scene=0).instances) == 1


def _material_doc(w, material, uv1=None, image=None, sampler=None, tex_extra=None):
    pos, tri = _quad()
    att = {"POSITION": w.accessor(pos), "TEXCOORD_0": w.accessor(np.zeros((5, 2), F))}
    if uv1 is not None:
        att["TEXCOORD_1"] = w.accessor(uv1)
    if image is not None:
        t = {"source": image}
        if sampler is not None:
            t["sampler"] = w.add("samplers", sampler)
        tex = dict({"index": w.add("textures", t), "texCoord": 1}, **(tex_extra or {}))
        material.setdefault("pbrMetallicRoughness", {})["baseColorTexture"] = tex
    mat = w.add("materials", material)
    _one_mesh(w, {"attributes": att, "indices": w.accessor(tri.reshape(-1), G.UBYTE), "material": mat})


def test_mask_material_with_png_alpha_on_texcoord_1(tmp_path):
    from rsd.gltf import load_gltf
    from rsd.scenes import FLAG_ALPHA_MASK, FLAG_DOUBLE_SIDED
    rgba = np.random.default_rng(3).integers(0, 256, (4, 4, 4)).astype(np.uint8)
    uv1 = np.array([[0.1, 0.2], [0.9, 0.2], [0.9, 0.8], [0.1, 0.8], [0.5, 0.5]], F)
    for embed in (True, False):
        w = G.Writer()
        _material_doc(w, {"alphaMode": "MASK", "alphaCutoff": 0.3, "doubleSided": True,
                          "pbrMetallicRoughness": {"baseColorFactor": [1, 1, 1, 0.75]}}, uv1,
                      w.image(G.png(rgba), embed=embed), sampler={"wrapS": 10497})
        s = load_gltf(w.save(tmp_path / f"m{int(embed)}.glb", "glb"))
        assert (s.flags == (FLAG_ALPHA_MASK | FLAG_DOUBLE_SIDED)).all()
        a = s.alpha
        assert a.thresholds.tolist() == [F(0.3)] and a.alphas.tolist() == [F(0.75)] and a.material_textures.tolist() == [0]
        assert np.array_equal(a.textures[0], rgba[..., 3]) and a.texcoords.tobytes() == uv1.tobytes()


def test_blend_opaque_and_jpeg(tmp_path):
    from rsd.gltf import load_gltf
    from rsd.scenes import FLAG_ALPHA_MASK, NO_TEXTURE
    w = G.Writer()
    _material_doc(w, {"alphaMode": "BLEND", "alphaCutoff": 0.9, "pbrMetallicRoughness": {"baseColorFactor": [1, 1, 1, 0.4]}})
    s = load_gltf(w.save(tmp_path / "b.gltf"))
    assert (s.flags == FLAG_ALPHA_MASK).all() and s.alpha.thresholds.tolist() == [0.5] and s.alpha.alphas.tolist() == [F(0.4)]
    w = G.Writer()
    _material_doc(w, {"alphaMode": "OPAQUE", "pbrMetallicRoughness": {"baseColorFactor": [1, 1, 1, 0.1]}})
    s = load_gltf(w.save(tmp_path / "o.gltf"))
    assert (s.flags == 0).all() and s.alpha is None
    # a JPEG base colour has no alpha channel: alpha 1 x the factor, no texture (only the SOI marker is looked at)
    w = G.Writer()
    _material_doc(w, {"alphaMode": "MASK"}, np.zeros((5, 2), F), w.image(b"\xff\xd8\xff\xe0" + bytes(16), "image/jpeg"))
    s = load_gltf(w.save(tmp_path / "j.gltf"))
    assert s.alpha.material_textures.tolist() == [NO_TEXTURE] and s.alpha.alphas.tolist() == [1.0]
    assert s.alpha.thresholds.tolist() == [0.5]


def test_refusals_name_the_offender(tmp_path):
    from rsd.gltf import GltfError, load_gltf
    pos, tri = _quad()
    img = G.png(np.full((2, 2, 4), 200, np.uint8))
    w = G.Writer()
    _material_doc(w, {"name": "leaf", "alphaMode": "MASK"}, np.zeros((5, 2), F), w.image(img),
                  tex_extra={"extensions": {"KHR_texture_transform": {"scale": [2, 2]}}})
    with pytest.raises(GltfError, match=r"material 0 \('leaf'\).*KHR_texture_transform"):
        load_gltf(w.save(tmp_path / "t.gltf"))
    w = G.Writer()
    _material_doc(w, {"name": "leaf", "alphaMode": "MASK"}, np.zeros((5, 2), F), w.image(img), sampler={"wrapT": 33071})
    with pytest.raises(GltfError, match=r"leaf.*wrapT 33071"):
        load_gltf(w.save(tmp_path / "w.gltf"))
    w = G.Writer()
    _material_doc(w, {"alphaMode": "MASK"}, np.zeros((5, 2), F), w.image(b"RIFF....WEBP", "image/webp"))
    w.doc["images"][0]["name"] = "bark"
    with pytest.raises(GltfError, match=r"image 0 \('bark'\).*image/webp"):
        load_gltf(w.save(tmp_path / "k.gltf"))
    w = G.Writer()
    _one_mesh(w, {"attributes": {"POSITION": w.accessor(pos)}, "indices": w.accessor(tri.reshape(-1), G.UBYTE)})
    w.doc["accessors"][0].update(name="thin", sparse={"count": 1, "indices": {"bufferView": 0, "componentType": G.UBYTE},
                                                       "values": {"bufferView": 0}})
    with pytest.raises(GltfError, match=r"accessor 0 \('thin'\) is sparse"):
        load_gltf(w.save(tmp_path / "s.gltf"))
    w = G.Writer()
    j = w.accessor(np.zeros((5, 4)), G.UBYTE)
    wt = w.accessor(np.tile(F([1, 0, 0, 0]), (5, 1)))
    _one_mesh(w, {"attributes": {"POSITION": w.accessor(pos), "JOINTS_0": j, "WEIGHTS_0": wt, "JOINTS_1": j, "WEIGHTS_1": wt}},
              name="octopus")
    with pytest.raises(GltfError, match=r"mesh 0 \('octopus'\) primitive 0 has JOINTS_1: more than 4 influences"):
        load_gltf(w.save(tmp_path / "j.gltf"))


def test_camera_node_and_default_framing(tmp_path):
    from rsd.gltf import load_gltf
    w, _ = gltf_scenes.cylinder()
    c = load_gltf(w.save(tmp_path / "c.gltf")).camera
    R = _trs(q=quat([1, 0, 0], -0.45))[:3, :3]
    assert np.allclose(c["pos"], [0.2, 1.6, 2.6]) and np.allclose(np.subtract(c["target"], c["pos"]), -R[:, 2])
    assert np.allclose(c["up"], R[:, 1]) and (c["yfov"], c["znear"], c["zfar"]) == (0.8, 0.1, 100.0)
    w, _ = gltf_scenes.cylinder(camera=False)
    c = load_gltf(w.save(tmp_path / "n.gltf")).camera
    assert np.allclose(c["target"], [0.0, 0.25, 0.0]) and c["pos"][2] > 2.0 and "yfov" not in c


# ---------------------------------------------------------------------------------- animation

def _slerp(a, b, u):
    """Specification appendix C: along the shortest arc."""
    d = float(np.dot(a, b))
    s = 1.0 if d >= 0 else -1.0
    ang = math.acos(abs(d))
    return (math.sin(ang * (1 - u)) * a + s * math.sin(ang * u) * b) / math.sin(ang)


def _cubic(t0, t1, v0, b0, v1, a1, t):
    td = t1 - t0
    u = (t - t0) / td
    return ((2 * u**3 - 3 * u**2 + 1) * v0 + td * (u**3 - 2 * u**2 + u) * b0 + (-2 * u**3 + 3 * u**2) * v1
            + td * (u**3 - u**2) * a1)


TIMES = [0.5, 1.0, 2.5]
TR = np.array([[0.0, 1.0, 2.0], [3.0, -1.0, 0.5], [-2.0, 0.25, 8.0]])
# the second and third keys have a negative dot product: the short way round
ROT = np.array([quat([0, 0, 1], 0.3), quat([0, 1, 0], 1.2), -quat([1, 1, 0], 2.0)])
TAN_T = np.array([[[1.0, 0, 0], [0, 2.0, 0]], [[0.5, 0.5, 0], [0, 0, -1.0]], [[0, 1.0, 1.0], [3.0, 0, 0]]])  # in, out
TAN_R = 0.3 * np.array([[[0, 0, 1.0, 0], [0, 1.0, 0, 0]], [[1.0, 0, 0, 0], [0, 0, 0, 1.0]], [[0, 1.0, 1.0, 0], [1.0, 0, 0, 1.0]]])
PROBES = [0.5, 1.0, 2.5, 0.75, 1.75, 0.1, 3.0]  # the keys, midway between keys, before and after the range


@pytest.fixture(scope="module")
def animated_nodes(tmp_path_factory):
    """One document: nodes 0..2 carry LINEAR, STEP and CUBICSPLINE translation + rotation channels; each keeps its
    static scale (no channel)."""
    from rsd.gltf import load_gltf_builder
    w = G.Writer()
    chans = []
    for n, interp in enumerate(("LINEAR", "STEP", "CUBICSPLINE")):
        w.add("nodes", G.trs_node([9, 9, 9], quat([1, 0, 0], 1.0), [1.0, 2.0, 3.0]))
        if interp == "CUBICSPLINE":
            vt = np.stack([TAN_T[:, 0], TR, TAN_T[:, 1]], 1)
            vr = np.stack([TAN_R[:, 0], ROT, TAN_R[:, 1]], 1)
        else:
            vt, vr = TR, ROT
        chans += [(n, "translation", TIMES, vt, interp), (n, "rotation", TIMES, vr, interp)]
    G.add_animation(w, chans[:2], "first")
    G.add_animation(w, chans[2:], "second")  # every animation of the file plays
    B = load_gltf_builder(w.save(tmp_path_factory.mktemp("anim") / "a.gltf"))
    return {a.nodeID: a for a in B.animations}, B


def _segment(t):
    tc = min(max(t, TIMES[0]), TIMES[-1])
    k = 0 if tc < TIMES[1] else 1
    return tc, k


@pytest.mark.parametrize("t", PROBES)
def test_linear_step_and_cubic_channels_match_closed_forms(animated_nodes, t):
    anims, _ = animated_nodes
    f32 = lambda a: np.asarray(a, F).astype(np.float64)  # noqa: E731 -- what the file stores
    tr, rot, tan_t, tan_r, times = f32(TR), f32(ROT), f32(TAN_T), f32(TAN_R), f32(TIMES)
    tc = min(max(t, times[0]), times[-1])
    k = 0 if tc < times[1] else 1
    u = (tc - times[k]) / (times[k + 1] - times[k])
    want = {
        0: ((1 - u) * tr[k] + u * tr[k + 1], _slerp(rot[k], rot[k + 1], u)),
        1: (tr[2] if tc >= times[2] else tr[k], rot[2] if tc >= times[2] else rot[k]),
        2: (_cubic(times[k], times[k + 1], tr[k], tan_t[k, 1], tr[k + 1], tan_t[k + 1, 0], tc),
            _cubic(times[k], times[k + 1], rot[k], tan_r[k, 1], rot[k + 1], tan_r[k + 1, 0], tc)),
    }
    for node, (wt, wr) in want.items():
        if node == 2:
            wr = wr / np.linalg.norm(wr)  # CUBICSPLINE rotations are normalised after interpolation
        a = anims[node]
        assert np.allclose(a.value("translation", t), wt, rtol=0, atol=1e-12), (node, t)
        got = a.value("rotation", t)
        got = got if np.dot(got, wr) >= 0 else -got  # q and -q are one rotation (at a key slerp gives sign * key)
        assert np.allclose(got, wr, rtol=0, atol=1e-12), (node, t)
        assert np.array_equal(a.value("scale", t), [1.0, 2.0, 3.0]), "a path without a channel keeps the node's value"
        assert np.allclose(a.animate(t), _trs(wt, wr, (1.0, 2.0, 3.0)), rtol=0, atol=1e-12)


def test_linear_rotation_takes_the_shortest_arc(animated_nodes):
    anims, _ = animated_nodes
    a, b = np.asarray(ROT[1], F).astype(np.float64), np.asarray(ROT[2], F).astype(np.float64)
    assert np.dot(a, b) < -0.1
    mid = anims[0].value("rotation", 1.75)
    assert np.dot(mid, a) > 0 and np.dot(mid, -b) > 0 and abs(np.linalg.norm(mid) - 1) < 1e-6
    long_way = (math.sin(0.5 * math.acos(np.dot(a, b))) * (a + b)) / math.sin(math.acos(np.dot(a, b)))
    assert not np.allclose(mid, long_way, atol=1e-3)


def test_animation_controller_consumes_the_gltf_animations(animated_nodes):
    from rsd.animation import AnimationController
    anims, B = animated_nodes
    c = AnimationController(B.nodes, B.animations, matrix_nodes=[0, 2])
    m = c.matrices(1.75)
    assert m.dtype == F and np.array_equal(m[0], anims[0].animate(1.75)[:3].astype(F).reshape(12))
    assert np.array_equal(m[1], anims[2].animate(1.75)[:3].astype(F).reshape(12))


# ---------------------------------------------------------------------------------- skins

def _cylinder_matrices(info, t):
    """G(joint) * IBM of the cylinder at time t from this file's own float64 evaluation, rounded once."""
    f32 = lambda a: np.asarray(a, F).astype(np.float64)  # noqa: E731
    at, av, bt, bv = f32(info["a_times"]), f32(info["a_values"]), f32(info["b_times"]), f32(info["b_values"])
    tc = min(max(t, at[0]), at[-1])
    ua = (tc - at[0]) / (at[1] - at[0])
    A = _trs((1 - ua) * av[0] + ua * av[1])
    tc = min(max(t, bt[0]), bt[-1])
    k = 0 if tc < bt[1] else 1
    q = _slerp(bv[k], bv[k + 1], (tc - bt[k]) / (bt[k + 1] - bt[k])) if tc > bt[0] else bv[0]
    Bm = A @ _trs((0.0, 0.5, 0.0), q)
    return np.stack([(A @ info["ibm"][0])[:3].astype(F).reshape(12), (Bm @ info["ibm"][1])[:3].astype(F).reshape(12)])


@pytest.mark.parametrize("t", gltf_scenes.CYL_TIMES)
def test_skin_matrices_are_global_times_inverse_bind(tmp_path, t):
    from rsd.gltf import load_gltf
    w, info = gltf_scenes.cylinder()
    s = load_gltf(w.save(tmp_path / "c.glb", "glb"))
    want = _cylinder_matrices(info, t)
    assert _u32(s.rig.matrices(t)).tobytes() == _u32(want).tobytes()
    assert np.array_equal(s.rig.matrix_ids, np.tile([0, 1, 0, 0], (16, 1))) and s.rig.matrix_count == 2
    assert np.array_equal(s.rig.weights, info["weights"]) and np.array_equal(s.rig.vertex_ids, np.arange(16))
    assert s.rig.rest.tobytes() == info["positions"].tobytes()


def test_the_skinned_mesh_nodes_own_transform_has_no_effect(tmp_path):
    from rsd.gltf import load_gltf
    a = load_gltf(gltf_scenes.cylinder()[0].save(tmp_path / "a.gltf"))
    b = load_gltf(gltf_scenes.cylinder(mesh_translation=(5.0, -3.0, 7.0))[0].save(tmp_path / "b.gltf"))
    assert a.positions.tobytes() == b.positions.tobytes() and a.rig.rest.tobytes() == b.rig.rest.tobytes()
    assert a.rig.matrices(0.4).tobytes() == b.rig.matrices(0.4).tobytes()


def test_unskinned_mesh_under_an_animated_node_is_a_rigid_rig_entry(tmp_path):
    from rsd.gltf import load_gltf
    pos, tri = _quad()
    w = G.Writer()
    mesh = w.add("meshes", {"primitives": [{"attributes": {"POSITION": w.accessor(pos)},
                                            "indices": w.accessor(tri.reshape(-1), G.UBYTE)}]})
    w.add("nodes", G.trs_node([1, 0, 0], children=[1]))
    w.add("nodes", G.trs_node([0, 2, 0], mesh=mesh))
    w.add("nodes", {"mesh": mesh})
    G.add_animation(w, [(0, "translation", [0.0, 2.0], [[1, 0, 0], [1, 4, 0]], "LINEAR")])
    s = load_gltf(w.save(tmp_path / "r.gltf"))
    assert s.rig.count == 5 and s.rig.morph is None and np.array_equal(s.rig.vertex_ids, np.arange(5))
    assert np.array_equal(s.rig.matrix_ids, np.zeros((5, 4))) and np.array_equal(s.rig.weights, np.tile(F([1, 0, 0, 0]), (5, 1)))
    assert np.array_equal(s.rig.matrices(1.0), F([[1, 0, 0, 1, 0, 1, 0, 4, 0, 0, 1, 0]]))


# ---------------------------------------------------------------------------------- routing

def test_pyscene_routes_gltf_and_glb(tmp_path):
    from rsd import pyscene
    w, _ = gltf_scenes.cylinder()
    w.save(tmp_path / "x.glb", "glb")
    pyscene._SCRIPT_DIR.append(tmp_path)
    try:
        m = pyscene.TriangleMesh.createFromFile("x.glb")
    finally:
        pyscene._SCRIPT_DIR.pop()
    assert len(m._p) == 20 and len(m._i) == 72
    w.save(tmp_path / "y.gltf")
    (tmp_path / "s.pyscene").write_text("sceneBuilder.importScene('y.gltf')\n")
    s = pyscene.load_pyscene(tmp_path / "s.pyscene").build()
    assert s.positions.shape == (20, 3) and s.rig.count == 16 and s.rig.morph.weight_count == 2
    assert pyscene.load_scene_file(tmp_path / "x.glb").build().positions.tobytes() == s.positions.tobytes()
