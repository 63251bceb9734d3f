"""CPU: keyframe animations, the node hierarchy and the rig a scene build produces (rsd.animation, rsd.pyscene,
rsd.ingest; DESIGN.md 4 "Animated scenes").  Expected matrices are composed here in float64 from the keyframes'
own translation / rotation / scaling; the evaluation is float64 too, so agreement is asked to 1e-12."""
import math

import numpy as np
import pytest

import skinning_checker
from conftest import ROOT

FIXTURES = ROOT / "tests" / "fixtures"


def _T(t=(0, 0, 0), deg=(0, 0, 0), s=(1, 1, 1)):
    from rsd.pyscene import Transform
    return Transform(translation=np.float32(t), rotationEulerDeg=np.float32(deg), scaling=np.float32(s))


def _trs(tr):
    """T * R * S of a Transform in float64, from its own fields."""
    x, y, z, w = (float(v) for v in tr.rotation)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    M = np.eye(4)
    M[:3, :3] = R @ np.diag(np.asarray(tr.scaling, np.float64))
    M[:3, 3] = np.asarray(tr.translation, np.float64)
    return M


def _anim(keys, duration=None, **kw):
    from rsd.animation import Animation
    a = Animation("a", 0, duration if duration is not None else max(t for t, _ in keys))
    for k, v in kw.items():
        setattr(a, k, v)
    for t, tr in keys:
        a.addKeyframe(t, tr)
    return a


def _keys5():
    return [(0.0, _T((0, 0, 0), (0, 0, 0))), (1.0, _T((1, 0, 2), (0, 40, 0), (1, 2, 1))), (2.0, _T((3, 1, 2), (30, 80, 0))),
            (3.0, _T((3, 2, -1), (30, 120, 20), (2, 2, 2))), (4.0, _T((0, 2, -1), (0, 160, 20)))]


@pytest.mark.parametrize("mode", ["Linear", "Hermite"])
def test_animate_returns_each_keyframe_at_its_time(mode):
    from rsd.animation import InterpolationMode
    keys = _keys5()
    a = _anim(keys, interpolationMode=InterpolationMode[mode])
    for t, tr in keys:
        assert np.allclose(a.animate(t), _trs(tr), rtol=0, atol=1e-12), (mode, t)


def test_linear_midpoint_and_a_90_degree_slerp():
    a = _anim([(0.0, _T((0, 0, 0), (0, 0, 0), (1, 1, 1))), (2.0, _T((2, -4, 6), (0, 90, 0), (3, 1, 1)))])
    M = a.animate(1.0)
    assert np.allclose(M[:3, 3], [1, -2, 3], rtol=0, atol=1e-12)
    # halfway through a quarter turn about y: 45 degrees, with the scaling (2, 1, 1) on the columns
    c = math.sqrt(0.5)
    want = np.array([[c, 0, c], [0, 1, 0], [-c, 0, c]]) @ np.diag([2.0, 1.0, 1.0])
    assert np.allclose(M[:3, :3], want, rtol=0, atol=1e-6)  # the keyframe's quaternion is float32 (Transform)
    q = a.animate(0.5)  # a quarter of the way: 22.5 degrees
    assert np.isclose(math.degrees(math.atan2(q[0, 2] / 1.0, q[2, 2] / 1.0)), 22.5, rtol=0, atol=1e-5)


def test_hermite_needs_four_keyframes():
    from rsd.animation import InterpolationMode
    keys = _keys5()
    lin3, her3 = _anim(keys[:3]), _anim(keys[:3], interpolationMode=InterpolationMode.Hermite)
    for t in np.linspace(0.0, 2.0, 9):
        assert np.array_equal(lin3.animate(t), her3.animate(t)), t
    lin5, her5 = _anim(keys), _anim(keys, interpolationMode=InterpolationMode.Hermite)
    for t, _ in keys:
        assert np.allclose(lin5.animate(t), her5.animate(t), rtol=0, atol=1e-12), t
    for t in (0.5, 1.5, 2.25, 3.5):
        assert np.abs(lin5.animate(t) - her5.animate(t)).max() > 1e-3, t
    # the scaling is lerped in both modes (keys that only scale; the spline's rotation is not renormalised, so it
    # would show in the column norms of keys that rotate)
    sk = [(float(i), _T(s=(v, 1, 1))) for i, v in enumerate((1, 2, 1, 3, 1))]
    ls, hs = _anim(sk), _anim(sk, interpolationMode=InterpolationMode.Hermite)
    assert np.allclose(ls.animate(2.25), hs.animate(2.25), rtol=0, atol=1e-12) and ls.animate(2.25)[0, 0] == 1.5


def test_behaviours_outside_the_keyframes():
    from rsd.animation import Behavior
    keys = [(1.0, _T((0, 0, 0))), (2.0, _T((2, 0, 0))), (3.0, _T((2, 4, 0)))]
    x = lambda a, t: a.animate(t)[:3, 3]  # noqa: E731
    const = _anim(keys, 3.0)
    assert np.array_equal(x(const, -5.0), [0, 0, 0]) and np.array_equal(x(const, 9.0), [2, 4, 0])
    cyc = _anim(keys, 3.0, preInfinityBehavior=Behavior.Cycle, postInfinityBehavior=Behavior.Cycle)
    assert np.allclose(x(cyc, 3.5), x(cyc, 1.5), atol=1e-12) and np.allclose(x(cyc, 1.5), [1, 0, 0], atol=1e-12)
    assert np.allclose(x(cyc, 7.75), x(cyc, 1.75), atol=1e-12)
    assert np.allclose(x(cyc, 0.5), x(cyc, 2.5), atol=1e-12) and np.allclose(x(cyc, -2.5), x(cyc, 1.5), atol=1e-12)
    osc = _anim(keys, 3.0, preInfinityBehavior=Behavior.Oscillate, postInfinityBehavior=Behavior.Oscillate)
    assert np.allclose(x(osc, 3.5), x(osc, 2.5), atol=1e-12) and np.allclose(x(osc, 5.5), x(osc, 1.5), atol=1e-12)
    assert np.allclose(x(osc, 0.5), x(osc, 1.5), atol=1e-12) and np.allclose(x(osc, -1.5), x(osc, 2.5), atol=1e-12)
    assert np.allclose(x(osc, -2.5), x(osc, 1.5), atol=1e-12)
    lin = _anim(keys, 3.0, preInfinityBehavior=Behavior.Linear, postInfinityBehavior=Behavior.Linear)
    # the end segments continue: slope (2, 0, 0) per second before the first key, (0, 4, 0) after the last;
    # the extrapolation runs through a point 1e-5 inside the range, which costs relative precision
    assert np.allclose(x(lin, 0.0), [-2, 0, 0], rtol=0, atol=1e-6) and np.allclose(x(lin, -1.5), [-5, 0, 0], rtol=0, atol=1e-6)
    assert np.allclose(x(lin, 4.0), [2, 8, 0], rtol=0, atol=1e-6) and np.allclose(x(lin, 3.25), [2, 5, 0], rtol=0, atol=1e-6)


def test_warping_wraps_the_last_segment():
    from rsd.animation import InterpolationMode
    keys = _keys5()
    plain, warp = _anim(keys, 5.0), _anim(keys, 5.0, enableWarping=True)
    # inside the keyframes Linear does not look past its segment: warping changes nothing
    assert np.array_equal(plain.animate(1.5), warp.animate(1.5))
    # the segment after the last keyframe leads back to the first one over duration - last = 1 second
    k = warp._interpolate(4.5)
    assert np.allclose(k.translation, [0, 1, -0.5], rtol=0, atol=1e-12)
    assert np.allclose(plain._interpolate(4.5).translation, [0, 2, -1], rtol=0, atol=1e-12)
    # Hermite's outer control points wrap too: the first segment sees the last keyframe instead of a clamped first one
    hp = _anim(keys, 5.0, interpolationMode=InterpolationMode.Hermite)
    hw = _anim(keys, 5.0, interpolationMode=InterpolationMode.Hermite, enableWarping=True)
    assert np.abs(hp.animate(0.5) - hw.animate(0.5)).max() > 1e-3
    assert np.allclose(hp.animate(1.5), hw.animate(1.5), rtol=0, atol=1e-12)


def test_a_keyframe_at_an_existing_time_replaces_it_and_inserts_stay_ordered():
    a = _anim([(2.0, _T((2, 0, 0))), (0.0, _T((0, 0, 0))), (1.0, _T((9, 9, 9))), (3.0, _T((3, 0, 0)))])
    a.addKeyframe(1.0, _T((1, 0, 0)))
    assert [k.time for k in a.keyframes] == [0.0, 1.0, 2.0, 3.0]
    assert np.array_equal(a.animate(1.0)[:3, 3], [1, 0, 0]) and np.allclose(a.animate(0.5)[:3, 3], [0.5, 0, 0], atol=1e-12)
    with pytest.raises(ValueError, match="duration"):
        a.addKeyframe(3.5, _T())


def test_a_child_moves_with_its_animated_parent():
    from rsd.animation import INVALID_ID, AnimationController
    parent, child, other = _T((1, 0, 0)).matrix, _T((0, 2, 0), (0, 0, 90)).matrix, _T((5, 5, 5)).matrix
    a = _anim([(0.0, _T((1, 0, 0))), (1.0, _T((1, 0, 4), (0, 90, 0)))])
    c = AnimationController([(parent, INVALID_ID), (child, 0), (other, INVALID_ID)], [a], matrix_nodes=[1, 2, 0])
    assert c.animated_nodes() == {0, 1}
    for t in (0.0, 0.25, 1.0):
        g = c.global_matrices(t)
        assert np.array_equal(g[0], a.animate(t)) and np.array_equal(g[2], other.astype(np.float64))
        assert np.allclose(g[1], a.animate(t) @ child.astype(np.float64), rtol=0, atol=1e-15)
        m = c.matrices(t)
        assert m.dtype == np.float32 and m.shape == (3, 12)
        assert np.array_equal(m[0], g[1][:3].astype(np.float32).reshape(12)), "rounded once, from float64"
        assert np.array_equal(m[2], g[0][:3].astype(np.float32).reshape(12))
    assert not np.array_equal(c.matrices(0.0)[0], c.matrices(1.0)[0])
    assert np.array_equal(c.matrices(0.0)[1], c.matrices(1.0)[1])


@pytest.fixture(scope="module")
def turnstile():
    from rsd.pyscene import load_pyscene
    B = load_pyscene(FIXTURES / "turnstile.pyscene")
    return B, B.build("turnstile")


def test_turnstile_rig_names_exactly_the_turnstile(turnstile):
    B, scene = turnstile
    rig = scene.rig
    assert rig is not None and len(B.animations) == 2
    # instances in script order: floor (4 vertices), post (24), four arms (24 each)
    assert scene.positions.shape[0] == 4 + 24 + 4 * 24
    assert np.array_equal(rig.vertex_ids, np.arange(28, 28 + 96, dtype=np.uint32))
    assert rig.matrix_count == 4 and np.array_equal(rig.matrix_ids[:, 0], np.repeat(np.arange(4, dtype=np.uint32), 24))
    assert not rig.matrix_ids[:, 1:].any() and np.array_equal(rig.weights, np.tile(np.float32([1, 0, 0, 0]), (96, 1)))
    assert rig.rest.shape == (96, 3) and np.array_equal(rig.rest[:24], B.meshes[2].positions)
    # every triangle index of an arm is inside the rig, none of the floor's or the post's is
    inside = np.isin(scene.indices, rig.vertex_ids).all(axis=1)
    assert inside.sum() == 4 * 12 and not np.isin(scene.indices[~inside], rig.vertex_ids).any()


def test_turnstile_pose_at_rest_time_is_the_soup(turnstile):
    _, scene = turnstile
    rig = scene.rig
    p0 = skinning_checker.posed(scene.positions, rig, rig.matrices(0.0))
    assert p0.tobytes() == scene.positions.tobytes()
    p1 = skinning_checker.posed(scene.positions, rig, rig.matrices(0.37))
    moved = (p1 != scene.positions).any(axis=1)
    assert moved[rig.vertex_ids].all() and not moved[:28].any()
    # the folding arm does not stay in the plane the three others turn in
    y = p1[:, 1].reshape(-1)
    assert np.ptp(y[28:28 + 72]) < 0.13 and np.ptp(y[28 + 72:]) > 0.15
    # past the last key the animations cycle
    assert np.allclose(rig.matrices(1.9), rig.matrices(0.4), rtol=0, atol=1e-6)
    assert not np.allclose(rig.matrices(1.9), rig.matrices(1.5), rtol=0, atol=1e-2)
    # rigid motion keeps the arms' edge lengths
    e = lambda p: np.linalg.norm(p[scene.indices[-48:, 0]] - p[scene.indices[-48:, 1]], axis=1)  # noqa: E731
    assert np.allclose(e(p1), e(scene.positions), rtol=0, atol=1e-5)


def test_pose_positions_is_the_checker(turnstile):
    """rsd.animation.pose_positions (what the build places animated instances with) against the checker's loop."""
    from rsd.animation import Rig, pose_positions
    rng = np.random.default_rng(3)
    n, nm = 200, 7
    rest = rng.standard_normal((n, 3)).astype(np.float32)
    rig = Rig(np.arange(n), rng.integers(0, nm, (n, 4)), rng.uniform(-0.2, 0.9, (n, 4)), nm, rest=rest)
    M = skinning_checker.random_matrices(rng, nm, translation=50.0)
    want = skinning_checker.posed(np.zeros((n, 3), np.float32), rig, M)
    assert pose_positions(rest, rig.matrix_ids, rig.weights, M).tobytes() == want.tobytes()


def test_a_scene_without_animations_builds_what_it_built_before():
    """courtyard.pyscene has nodes and no animation: its build is the still build, byte for byte, and has no rig."""
    from rsd.pyscene import load_pyscene
    B = load_pyscene(FIXTURES / "courtyard.pyscene")
    assert B.nodes and not B.animations
    a, b = B.build("courtyard"), B.build("courtyard", animated=False)
    assert a.rig is None and b.rig is None
    for f in ("positions", "indices", "flags"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes() and getattr(a, f).dtype == getattr(b, f).dtype, f
    # and the still build of an animated scene is the same soup up to the arithmetic of the animated instances
    T = load_pyscene(FIXTURES / "turnstile.pyscene")
    still, moving = T.build("t", animated=False), T.build("t")
    assert still.rig is None and moving.rig is not None
    assert np.array_equal(still.indices, moving.indices) and np.array_equal(still.flags, moving.flags)
    assert still.positions[:28].tobytes() == moving.positions[:28].tobytes()
    assert np.allclose(still.positions, moving.positions, rtol=0, atol=1e-5)


def test_create_animation_makes_a_node_for_an_animatable():
    from rsd.pyscene import Camera, PySceneBuilder
    sb = PySceneBuilder()
    cam = Camera()
    a = sb.createAnimation(cam, "CamPath", 2.0)
    assert a is not None and a.nodeID == cam.nodeID == 0 and sb._B.animations == [a]
    assert sb.createAnimation(cam, "Again", 2.0) is None
    a.addKeyframe(0.0, _T())
    assert sb.finish().build("empty").positions.shape == (0, 3)
