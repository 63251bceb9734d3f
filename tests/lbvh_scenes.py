"""The scenes of the LBVH tests (tests/test_lbvh.py, tests/test_gpu_lbvh.py): the set of tests/test_bvh_refit.py plus
the shapes at which a Morton-code builder degenerates, and the motions a rebuild is meant for."""
import numpy as np

from test_bvh_refit import SCENES as REFIT_SCENES, _scene as _refit_scene

CAM = dict(pos=[0.0, 0.0, 3.0], target=[0.0, 0.0, 0.0], up=[0.0, 1.0, 0.0])
SMALL = REFIT_SCENES + ["coincident", "planar"]
SCENES = SMALL + ["arcade_50k"]


def scene(name):
    from rsd.scenes import Scene, make_scene
    if name == "coincident":  # 37 copies of one triangle: every code equal, the primitive id alone shapes the tree
        n = 37
        p = np.tile(np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0.5]], np.float32), (n, 1))
        t = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
        return Scene(name, p, t, np.zeros(n, np.uint32), CAM)
    if name == "planar":  # a 9 x 7 grid in the plane z = 0.25: one axis of zero extent
        xs, ys = np.meshgrid(np.linspace(-1.5, 1.5, 10, dtype=np.float32), np.linspace(-1, 1, 8, dtype=np.float32))
        p = np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, 0.25, np.float32)], 1).astype(np.float32)
        i = np.arange(80).reshape(8, 10)
        a, b, c, d = i[:-1, :-1], i[:-1, 1:], i[1:, 1:], i[1:, :-1]
        t = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 2).reshape(-1, 3).astype(np.uint32)
        return Scene(name, np.ascontiguousarray(p), np.ascontiguousarray(t), np.ones(t.shape[0], np.uint32), CAM)
    if name == "arcade_50k":  # thousands of wide nodes: every launch of the rebuild spans many workgroups
        return make_scene("arcade_tiny", target_tris=50_000)
    return _refit_scene(name)


def moved(s, seed, part=(0.4, 0.3, -0.5)):
    """tests/test_gpu_scene_update.py's motion: per-vertex jitter plus the last eighth of the triangles translated."""
    rng = np.random.default_rng(seed)
    p = s.positions + (0.02 * rng.standard_normal(s.positions.shape)).astype(np.float32)
    v = np.unique(s.indices[-max(1, s.indices.shape[0] // 8):])
    p[v] += np.float32(part)
    return np.ascontiguousarray(p, np.float32)


def large_motion(s):
    """A motion a refit decays under: the last quarter of the triangles crosses the scene (twice its extent in x),
    everything jitters."""
    ext = float(np.ptp(s.positions[:, 0])) or 1.0
    rng = np.random.default_rng(11)
    p = s.positions + (0.02 * rng.standard_normal(s.positions.shape)).astype(np.float32)
    v = np.unique(s.indices[-max(1, s.indices.shape[0] // 4):])
    p[v] += np.float32([2.0 * ext, -0.5 * ext, 0.25 * ext])
    return np.ascontiguousarray(p, np.float32)
