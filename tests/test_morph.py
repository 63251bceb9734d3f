"""CPU: morph targets from glTF to the rig's table (rsd/gltf.py, rsd.animation.MorphTable, Rig.morph_weights) and the
morph arithmetic on the host (rsd.animation.morph_positions against tests/morph_checker.py).  The device side:
tests/test_gpu_morph.py."""
import numpy as np
import pytest

import gltf_scenes
import gltf_writer as G
import morph_checker
import skinning_checker

F = np.float32


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def cylinder(tmp_path_factory):
    from rsd.gltf import load_gltf
    w, info = gltf_scenes.cylinder()
    return load_gltf(w.save(tmp_path_factory.mktemp("morph") / "c.glb", "glb")), info, w


def test_csr_table_leaves_out_zero_deltas(cylinder):
    s, info, _ = cylinder
    m = s.rig.morph
    off, ids, deltas = morph_checker.table_from_targets(info["targets"])
    assert m.count == s.rig.count == 16 and m.weight_count == 2
    assert np.array_equal(m.offsets, off) and np.array_equal(m.weight_ids, ids)
    assert _u32(m.deltas).tobytes() == _u32(deltas).tobytes()
    # the bottom ring has no entry of target 0; vertex 3's -0 delta of target 1 is no entry; vertex 9 has both
    counts = np.diff(m.offsets.astype(np.int64))
    assert counts[:8].tolist() == [0, 1, 0, 0, 0, 1, 0, 1] and counts[8:].tolist() == [1, 2] * 4
    assert m.entry_count == 15 and (np.abs(m.deltas).max(axis=1) > 0).all()


def test_default_weights_node_over_mesh_and_the_weights_channel(cylinder, tmp_path):
    from rsd.gltf import load_gltf
    s, info, w = cylinder
    wt, wv = np.asarray(info["w_times"]), np.asarray(info["w_values"], F).astype(np.float64)
    for t, want in ((-1.0, wv[0]), (0.0, wv[0]), (0.25, 0.5 * wv[0] + 0.5 * wv[1]), (0.5, wv[1]),
                    (0.75, 0.5 * wv[1] + 0.5 * wv[2]), (1.0, wv[2]), (9.0, wv[2])):
        got = s.rig.morph_weights(t)
        assert got.dtype == F and np.array_equal(got, want.astype(F)), t
    # without the channel: node.weights; without node.weights: mesh.weights; without either: zeros
    doc = w.doc
    saved = doc["animations"].pop()
    try:
        assert load_gltf(w.save(tmp_path / "n.gltf")).rig.morph_weights(0.3).tolist() == [0.75, 0.25]
        node_w = doc["nodes"][2].pop("weights")
        assert load_gltf(w.save(tmp_path / "m.gltf")).rig.morph_weights(0.3).tolist() == [0.5, 0.25]
        mesh_w = doc["meshes"][0].pop("weights")
        assert load_gltf(w.save(tmp_path / "z.gltf")).rig.morph_weights(0.3).tolist() == [0.0, 0.0]
        doc["meshes"][0]["weights"], doc["nodes"][2]["weights"] = mesh_w, node_w
    finally:
        doc["animations"].append(saved)


def test_step_and_cubic_weight_channels(tmp_path):
    from rsd.gltf import load_gltf
    w, _ = gltf_scenes.cylinder()
    w.doc["animations"].pop()
    v = np.array([[[0.0, 0.0], [0.25, 1.0], [1.0, -1.0]], [[2.0, 0.5], [0.75, 0.0], [0.0, 0.0]]])  # in, value, out x 2 keys
    G.add_animation(w, [(2, "weights", [0.0, 2.0], v, "CUBICSPLINE")])
    got = load_gltf(w.save(tmp_path / "c.gltf")).rig.morph_weights(0.5)
    u, td = 0.25, 2.0
    want = ((2 * u**3 - 3 * u**2 + 1) * v[0, 1] + td * (u**3 - 2 * u**2 + u) * v[0, 2] + (-2 * u**3 + 3 * u**2) * v[1, 1]
            + td * (u**3 - u**2) * v[1, 0])
    assert np.array_equal(got, want.astype(F))
    w.doc["animations"].pop()
    G.add_animation(w, [(2, "weights", [0.0, 2.0], [[0.25, 1.0], [0.75, 0.0]], "STEP")])
    rig = load_gltf(w.save(tmp_path / "s.gltf")).rig
    assert rig.morph_weights(1.99).tolist() == [0.25, 1.0] and rig.morph_weights(2.0).tolist() == [0.75, 0.0]


@pytest.mark.parametrize("t", gltf_scenes.CYL_TIMES)
def test_host_morph_arithmetic_matches_the_checker(cylinder, t):
    from rsd.animation import morph_positions, pose_positions
    s, _, _ = cylinder
    rig, m = s.rig, s.rig.morph
    wts, M = rig.morph_weights(t), rig.matrices(t)
    want = morph_checker.posed(s.positions, rig, M, m.offsets, m.weight_ids, m.deltas, wts)
    got = pose_positions(morph_positions(rig.rest, m, wts), rig.matrix_ids, rig.weights, M)
    assert _u32(got).tobytes() == _u32(want[rig.vertex_ids]).tobytes()
    assert not np.array_equal(want, skinning_checker.posed(s.positions, rig, M)), "the morph does not show"
    if t == 0.0:
        assert _u32(want).tobytes() == _u32(s.positions).tobytes(), "the pose at the rest time is the soup"


def test_a_morphed_static_mesh_enters_the_rig_as_a_rigid_entry(tmp_path):
    from rsd.gltf import load_gltf
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    d = np.array([[0, 0, 0], [0, 0, 0.5], [0, 0, 0]], F)
    w = G.Writer()
    mesh = w.add("meshes", {"weights": [2.0], "primitives": [{"attributes": {"POSITION": w.accessor(pos)},
                                                              "targets": [{"POSITION": w.accessor(d)}]}]})
    w.add("nodes", G.trs_node([0, 0, 3], mesh=mesh))
    w.add("nodes", G.trs_node([4, 0, 0], mesh=mesh, weights=[-1.0]))
    s = load_gltf(w.save(tmp_path / "m.gltf"))
    rig = s.rig
    assert rig.count == 6 and rig.matrix_count == 2 and rig.morph.weight_count == 2
    assert np.array_equal(rig.matrix_ids[:, 0], [0, 0, 0, 1, 1, 1]) and np.array_equal(rig.weights[:, 0], np.ones(6))
    assert rig.morph.offsets.tolist() == [0, 0, 1, 1, 1, 2, 2] and rig.morph.weight_ids.tolist() == [0, 1]
    assert rig.morph_weights(0.0).tolist() == [2.0, -1.0]
    assert s.positions.tolist() == [[0, 0, 3], [1, 0, 4], [0, 1, 3], [4, 0, 0], [5, 0, -0.5], [4, 1, 0]]
    assert load_gltf(tmp_path / "m.gltf", animated=False).rig is None


def test_morph_table_and_rig_check_their_shapes():
    from rsd.animation import MorphTable, Rig
    m = MorphTable([0, 1, 1], [0], [[1, 2, 3]], 1)
    assert (m.count, m.entry_count, m.weight_count) == (2, 1, 1)
    one = F([[1, 0, 0, 0]])
    assert Rig([4, 7], np.zeros((2, 4)), np.tile(one, (2, 1)), 1, morph=m).morph is m
    with pytest.raises(ValueError, match="morph table covers 2"):
        Rig([4], np.zeros((1, 4)), one, 1, morph=m)
    with pytest.raises(ValueError, match="no morph table"):
        Rig([4], np.zeros((1, 4)), one, 1).morph_weights(0.0)


def _zero_target_doc():
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    d = np.zeros((3, 3), F)
    d[1, 2] = F(-0.0)
    w = G.Writer()
    mesh = w.add("meshes", {"weights": [1.0], "primitives": [{"attributes": {"POSITION": w.accessor(pos)},
                                                              "targets": [{"POSITION": w.accessor(d)}]}]})
    w.add("nodes", G.trs_node([0, 0, 3], mesh=mesh))
    return w


def test_a_target_of_zero_deltas_gives_a_table_without_entries(tmp_path):
    """Every delta +-0: the rig is rigid on its node, its table has no entry, and the posing calls treat it as a rig
    without a table (rsd_scene_attach_morph would detach on it)."""
    from rsd.frame import rig_has_morph
    from rsd.gltf import load_gltf
    s = load_gltf(_zero_target_doc().save(tmp_path / "z.gltf"))
    assert s.rig.count == 3 and s.rig.morph.entry_count == 0 and s.rig.morph.offsets.tolist() == [0, 0, 0, 0]
    assert s.rig.morph_weights(0.0).tolist() == [1.0] and not rig_has_morph(s.rig)
    assert s.positions.tolist() == [[0, 0, 3], [1, 0, 3], [0, 1, 3]]


def test_import_into_a_builder_keeps_its_camera(tmp_path):
    from rsd.gltf import load_gltf_builder
    from rsd.ingest import SceneBuilder
    B = SceneBuilder()
    B.set_camera([1, 2, 3], [4, 5, 6])
    kept = dict(B.camera)
    load_gltf_builder(_zero_target_doc().save(tmp_path / "z.gltf"), builder=B)
    assert B.camera == kept, "a file without a camera leaves the builder's camera alone"
    w, _ = gltf_scenes.cylinder()
    load_gltf_builder(w.save(tmp_path / "c.gltf"), builder=B)
    assert B.camera["pos"] == [0.2, 1.6, 2.6], "a file's own camera is taken"
