"""Animated scenes on the host: keyframed node transforms, the node hierarchy and rigs (DESIGN.md 4 "Animated scenes").

Reference: Scene/Animation/Animation.cpp (`Animation::animate` :114-156, `interpolate` :158-219, `calcSampleTime`
:225-254, `addKeyframe` :256-295 and the script binding :321-351) and AnimationController.cpp
(`updateLocalMatrices` :289-298, `updateWorldMatrices` :300-329).  What is restated here:

* `Animation(name, nodeID, duration)`: keyframes of (time, translation, scaling, rotation quaternion) kept in time
  order, a keyframe at an existing time replacing it; `interpolationMode` (Linear, Hermite -- the Bezier-form spline
  on translation and rotation with the scaling lerped, Linear below 4 keyframes), `preInfinityBehavior` /
  `postInfinityBehavior` (Constant, Linear -- extrapolated through a point kEpsilonTime inside the range --, Cycle,
  Oscillate), `enableWarping`; `animate(t)` returns T * R * S.
* `AnimationController`: an animated node's local matrix is its animation's, global = parent's global * local.
* `Rig`: which vertices of a scene move, by which matrices and weights (rsd_rig_desc).

The reference computes in float.  Here everything is evaluated in float64 and each matrix element is rounded to
float32 once, at the end (`AnimationController.matrices`): the project's rule for matrices built on the host.
Bit parity with a Falcor run is therefore not claimed and not pinned by fixtures.  The evaluation stays on the
host; the GPU gets `matrix_count` x 12 floats per frame (rsd_scene_update_pose)."""
from __future__ import annotations

import dataclasses
import enum
import math

import numpy as np

INVALID_ID = 0xFFFFFFFF
K_EPSILON_TIME = float(np.float32(1e-5))  # `const double kEpsilonTime = 1e-5f`
_SLERP_EPS = float(np.finfo(np.float32).eps)  # slerp's lerp fall-back threshold (QuaternionMath.h:284, T = float)


class InterpolationMode(enum.Enum):
    Linear = 0
    Hermite = 1


class Behavior(enum.Enum):
    Constant = 0
    Linear = 1
    Cycle = 2
    Oscillate = 3


def _lerp(a, b, t):
    return a + (b - a) * t  # math::lerp


def _slerp(q1, q2, t):
    """QuaternionMath.h:269-295; quaternions are (x, y, z, w)."""
    c = float(np.dot(q1, q2))
    if c < 0.0:
        q2, c = -q2, -c
    if c > 1.0 - _SLERP_EPS:
        return _lerp(q1, q2, t)
    angle = math.acos(c)
    return (math.sin((1.0 - t) * angle) * q1 + math.sin(t * angle) * q2) / math.sin(angle)


def _hermite(p0, p1, p2, p3, t, mix):
    """Animation.cpp:50-83: the Bezier form of the Hermite spline, `mix` = lerp or slerp."""
    b0, b1, b2, b3 = p1, p1 + (p2 - p0) * 0.5 / 3.0, p2 - (p3 - p1) * 0.5 / 3.0, p2
    q0, q1, q2 = mix(b0, b1, t), mix(b1, b2, t), mix(b2, b3, t)
    return mix(mix(q0, q1, t), mix(q1, q2, t), t)


def matrix_from_quat(q) -> np.ndarray:
    """MatrixMath.h:715-741 in float64 (3x3)."""
    x, y, z, w = (float(v) for v in q)
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]], np.float64)


def compose_trs(translation, rotation, scaling) -> np.ndarray:
    """T * R * S as a float64 4x4 acting on column vectors."""
    M = np.eye(4, dtype=np.float64)
    M[:3, :3] = matrix_from_quat(rotation) * np.asarray(scaling, np.float64)[None, :]
    M[:3, 3] = np.asarray(translation, np.float64)
    return M


@dataclasses.dataclass
class Keyframe:
    time: float
    translation: np.ndarray  # float64 [3]
    scaling: np.ndarray      # float64 [3]
    rotation: np.ndarray     # float64 [4], (x, y, z, w)


def _interpolate_linear(k0: Keyframe, k1: Keyframe, t: float) -> Keyframe:
    """Animation.cpp:86-94; extrapolates when t is outside [0, 1]."""
    return Keyframe(_lerp(k0.time, k1.time, t), _lerp(k0.translation, k1.translation, t),
                    _lerp(k0.scaling, k1.scaling, t), _slerp(k0.rotation, k1.rotation, t))


class Animation:
    """Falcor's scripting surface of Animation (Animation.cpp:321-351)."""

    InterpolationMode = InterpolationMode
    Behavior = Behavior

    def __init__(self, name, nodeID, duration):
        self.name = str(name)
        self.nodeID = int(nodeID)
        self.duration = float(duration)
        self.preInfinityBehavior = Behavior.Constant
        self.postInfinityBehavior = Behavior.Constant
        self.interpolationMode = InterpolationMode.Linear
        self.enableWarping = False
        self.keyframes: list[Keyframe] = []

    def addKeyframe(self, time, transform):
        """:256-295 -- `transform`: anything with translation, scaling and rotation (x, y, z, w), rsd.pyscene.Transform."""
        time = float(time)
        if time > self.duration:
            raise ValueError(f"addKeyframe: time {time} is past the animation's duration {self.duration}")
        k = Keyframe(time, np.array(transform.translation, np.float64).reshape(3),
                     np.array(transform.scaling, np.float64).reshape(3), np.array(transform.rotation, np.float64).reshape(4))
        ks = self.keyframes
        for i, cur in enumerate(ks):
            if cur.time == time:
                ks[i] = k
                return
            if cur.time > time:
                ks.insert(i, k)
                return
        ks.append(k)

    def _sample_time(self, t: float) -> float:
        """calcSampleTime :225-254, for t outside the keyframes' range."""
        first, last = self.keyframes[0].time, self.keyframes[-1].time
        duration = last - first
        behavior = self.preInfinityBehavior if t < first else self.postInfinityBehavior
        if behavior == Behavior.Constant:
            return min(max(t, first), last)
        if duration <= 0.0:
            return first if behavior != Behavior.Linear else t  # one keyframe: nothing to cycle through
        if behavior == Behavior.Cycle:
            m = first + math.fmod(t - first, duration)
            return m + duration if m < first else m
        if behavior == Behavior.Oscillate:
            off = math.fmod(t - first, 2.0 * duration)
            if off < 0.0:
                off += 2.0 * duration
            if off > duration:
                off = 2.0 * duration - off
            return first + off
        return t  # Linear: the caller extrapolates

    def _interpolate(self, time: float) -> Keyframe:
        """interpolate :158-219 (the cached frame index is an optimisation there: the search result is the same)."""
        ks, n = self.keyframes, len(self.keyframes)
        frame = 0
        while frame < n - 1 and ks[frame + 1].time <= time:
            frame += 1

        def adjacent(f, offset=1):
            return (f + n + offset) % n if self.enableWarping else min(max(f + offset, 0), n - 1)

        def param(k0, k1):
            seg = k1.time - k0.time
            if self.enableWarping and seg < 0.0:
                seg += self.duration
            return min(max((time - k0.time) / seg if seg > 0.0 else 1.0, 0.0), 1.0)

        if self.interpolationMode == InterpolationMode.Linear or n < 4:
            k0, k1 = ks[frame], ks[adjacent(frame)]
            return _interpolate_linear(k0, k1, param(k0, k1))
        k0, k1, k2, k3 = ks[adjacent(frame, -1)], ks[frame], ks[adjacent(frame, 1)], ks[adjacent(frame, 2)]
        t = param(k1, k2)
        return Keyframe(_lerp(k1.time, k2.time, t), _hermite(k0.translation, k1.translation, k2.translation, k3.translation, t, _lerp),
                        _lerp(k1.scaling, k2.scaling, t), _hermite(k0.rotation, k1.rotation, k2.rotation, k3.rotation, t, _slerp))

    def animate(self, currentTime) -> np.ndarray:
        """Animation::animate :114-156: the node's local matrix at `currentTime`, float64 4x4."""
        if not self.keyframes:
            raise ValueError(f"Animation '{self.name}' has no keyframes")
        ks, time = self.keyframes, float(currentTime)
        if time < ks[0].time or time > ks[-1].time:
            time = self._sample_time(time)
        if time < ks[0].time and self.preInfinityBehavior == Behavior.Linear and len(ks) > 1:
            k0, k1 = ks[0], self._interpolate(ks[0].time + K_EPSILON_TIME)
            k = _interpolate_linear(k0, k1, (time - k0.time) / (k1.time - k0.time))
        elif time > ks[-1].time and self.postInfinityBehavior == Behavior.Linear and len(ks) > 1:
            k1, k0 = ks[-1], self._interpolate(ks[-1].time - K_EPSILON_TIME)
            k = _interpolate_linear(k0, k1, (time - k0.time) / (k1.time - k0.time))
        else:
            k = self._interpolate(time)
        return compose_trs(k.translation, k.rotation, k.scaling)


class AnimationController:
    """The scene graph and its animations: `nodes` is a list of (local matrix 4x4, parent id or INVALID_ID), parents
    before children; `matrix_nodes` names the nodes whose global matrices a pose consists of, in matrix order."""

    def __init__(self, nodes, animations, matrix_nodes=(), matrix_binds=None):
        """`animations`: anything with `.nodeID` and `.animate(t)` -> local 4x4 (Animation, rsd.gltf.NodeAnimation).
        matrix_binds: per matrix a float64 4x4 the node's global matrix is multiplied with on the right -- a skin's
        inverse bind matrix -- or None for the global matrix itself; None: no matrix has one."""
        self.nodes = [(np.asarray(m, np.float64).reshape(4, 4), int(p)) for m, p in nodes]
        self.animations = list(animations)
        self.matrix_nodes = [int(n) for n in matrix_nodes]
        self.matrix_binds = None if matrix_binds is None else list(matrix_binds)
        for i, (_, p) in enumerate(self.nodes):
            if p != INVALID_ID and not 0 <= p < i:
                raise ValueError(f"node {i}: parent {p} must come before it")
        for a in self.animations:
            if not 0 <= a.nodeID < len(self.nodes):
                raise ValueError(f"Animation '{a.name}': node {a.nodeID} does not exist")

    def animated_nodes(self) -> set:
        """Nodes whose chain to the root holds an animated node."""
        own = {a.nodeID for a in self.animations}
        out = set()
        for i, (_, p) in enumerate(self.nodes):
            if i in own or p in out:
                out.add(i)
        return out

    def global_matrices(self, t) -> list:
        """updateLocalMatrices + updateWorldMatrices at time t, float64 4x4 per node (a later animation of a node wins,
        as in the reference's loop)."""
        local = [m for m, _ in self.nodes]
        for a in self.animations:
            local[a.nodeID] = a.animate(t)
        out = []
        for i, (_, p) in enumerate(self.nodes):
            out.append(local[i] if p == INVALID_ID else out[p] @ local[i])
        return out

    def matrices(self, t) -> np.ndarray:
        """The pose at time t: float32 [len(matrix_nodes), 12], each element rounded once."""
        g = self.global_matrices(t)
        out = np.zeros((len(self.matrix_nodes), 12), np.float32)
        binds = self.matrix_binds
        for k, n in enumerate(self.matrix_nodes):
            m = g[n] if binds is None or binds[k] is None else g[n] @ binds[k]
            out[k] = m[:3, :].astype(np.float32).reshape(12)
        return out


class MorphTable:
    """rsd_morph_desc on the host: per rig vertex a run of (weight id, delta) entries in CSR form -- `offsets`
    [count + 1], `weight_ids` [entries], `deltas` [entries, 3] -- into a table of `weight_count` weights.
    `sources`: where the weights of time t come from, a list of (first weight id, default weights float64 [k],
    channel or None); a channel is anything with `.weights(t)` -> k values (rsd.gltf.WeightAnimation)."""

    def __init__(self, offsets, weight_ids, deltas, weight_count, sources=()):
        self.offsets = np.ascontiguousarray(offsets, np.uint32).reshape(-1)
        n = int(self.offsets[-1]) if self.offsets.size else 0
        self.weight_ids = np.ascontiguousarray(weight_ids, np.uint32).reshape(n)
        self.deltas = np.ascontiguousarray(deltas, np.float32).reshape(n, 3)
        self.weight_count = int(weight_count)
        self.sources = list(sources)

    @property
    def count(self) -> int:
        return max(int(self.offsets.size) - 1, 0)

    @property
    def entry_count(self) -> int:
        return int(self.weight_ids.size)

    @staticmethod
    def from_targets(blocks, sources=()) -> "MorphTable":
        """blocks: per run of rig vertices (n, first weight id, targets) with targets a list of float32 [n, 3] deltas
        or None for vertices without targets.  Target k of a vertex becomes an entry only if a component of its
        delta is not +-0; a vertex's entries are in target order."""
        counts, ids, deltas, nw = [], [], [], 0
        for n, base, targets in blocks:
            if not targets:
                counts.append(np.zeros(n, np.int64))
                continue
            d = np.stack([np.asarray(t, np.float32).reshape(n, 3) for t in targets], 1)  # [n, k, 3]
            live = (d != 0.0).any(axis=2)  # -0.0 != 0.0 is false: +-0 deltas drop out
            v, k = np.nonzero(live)        # row-major: by vertex, then by target
            counts.append(live.sum(axis=1))
            ids.append((base + k).astype(np.uint32))
            deltas.append(d[v, k])
            nw = max(nw, base + d.shape[1])
        nw = max([nw] + [b + len(w) for b, w, _ in sources])
        off = np.concatenate([[0], np.cumsum(np.concatenate(counts) if counts else np.zeros(0, np.int64))])
        return MorphTable(off, np.concatenate(ids) if ids else np.zeros(0, np.uint32),
                          np.concatenate(deltas) if deltas else np.zeros((0, 3), np.float32), nw, sources)

    def weights(self, t) -> np.ndarray:
        """The weight table at time t, float32 [weight_count]: evaluated in float64 and rounded once."""
        w = np.zeros(self.weight_count, np.float64)
        for base, default, channel in self.sources:
            w[base:base + len(default)] = default if channel is None else channel.weights(t)
        return w.astype(np.float32)


class Rig:
    """rsd_rig_desc on the host: `vertex_ids` [count] name the animated vertices of a scene, `matrix_ids` [count, 4]
    and `weights` [count, 4] their influences into a table of `matrix_count` matrices.  `rest` [count, 3]: the
    positions the matrices act on (None: the scene's positions when the rig is attached).  `controller`: an
    AnimationController whose matrices(t) is this rig's pose at time t (None for a rig posed by the caller).
    A rigid vertex of matrix m is ids (m, 0, 0, 0), weights (1, 0, 0, 0).  `morph`: a MorphTable over the rig's
    vertices (rsd_morph_desc), or None."""

    def __init__(self, vertex_ids, matrix_ids, weights, matrix_count, rest=None, controller=None, morph=None):
        self.vertex_ids = np.ascontiguousarray(vertex_ids, np.uint32).reshape(-1)
        n = self.vertex_ids.size
        self.matrix_ids = np.ascontiguousarray(matrix_ids, np.uint32).reshape(n, 4)
        self.weights = np.ascontiguousarray(weights, np.float32).reshape(n, 4)
        self.matrix_count = int(matrix_count)
        self.rest = None if rest is None else np.ascontiguousarray(rest, np.float32).reshape(n, 3)
        self.controller = controller
        if morph is not None and morph.count != n:
            raise ValueError(f"Rig: the morph table covers {morph.count} vertices, the rig has {n}")
        self.morph = morph

    def morph_weights(self, t) -> np.ndarray:
        """The morph weights at time t, float32 [morph.weight_count]."""
        if self.morph is None:
            raise ValueError("this rig has no morph table")
        return self.morph.weights(t)

    @property
    def count(self) -> int:
        return int(self.vertex_ids.size)

    @staticmethod
    def rigid(vertex_ids, matrix_of_vertex, matrix_count, rest=None, controller=None) -> "Rig":
        """Every vertex follows one matrix with weight 1."""
        v = np.asarray(vertex_ids, np.uint32).reshape(-1)
        ids = np.zeros((v.size, 4), np.uint32)
        ids[:, 0] = np.asarray(matrix_of_vertex, np.uint32).reshape(-1)
        w = np.zeros((v.size, 4), np.float32)
        w[:, 0] = 1.0
        return Rig(v, ids, w, matrix_count, rest, controller)

    def matrices(self, t) -> np.ndarray:
        if self.controller is None:
            raise ValueError("this rig has no animation controller: pose it with update_pose(matrices)")
        return self.controller.matrices(t)


def morph_positions(rest, morph: MorphTable, weights) -> np.ndarray:
    """rsd_scene_update_pose_morph's morph sum on the host in float32: per rig vertex, for its entries in ascending
    order, p = p + (w[id] * delta), the product rounded, then the sum.  What pose_positions is then given in place
    of the rest positions."""
    F = np.float32
    p = np.array(rest, F).reshape(-1, 3)
    w = np.asarray(weights, F).reshape(-1)
    off = morph.offsets.astype(np.int64)
    n = off[1:] - off[:-1]
    for k in range(int(n.max()) if n.size else 0):
        v = np.flatnonzero(n > k)
        e = off[v] + k
        p[v] = p[v] + (w[morph.weight_ids[e]][:, None] * morph.deltas[e]).astype(F)
    return p


def pose_positions(rest, matrix_ids, weights, matrices) -> np.ndarray:
    """rsd_scene_update_pose's arithmetic on the host in float32, every product and sum rounded on its own:
    B = ((M[i0] w0 + M[i1] w1) + M[i2] w2) + M[i3] w3 per element, out_r = ((B_r0 x + B_r1 y) + B_r2 z) + B_r3.
    Used by SceneBuilder.build to place animated instances, so that the pose at the rest time reproduces the
    soup bit for bit."""
    F = np.float32
    rest = np.asarray(rest, F).reshape(-1, 3)
    ids = np.asarray(matrix_ids, np.uint32).reshape(-1, 4)
    w = np.asarray(weights, F).reshape(-1, 4)
    M = np.asarray(matrices, F).reshape(-1, 12)
    B = ((M[ids[:, 0]] * w[:, 0:1] + M[ids[:, 1]] * w[:, 1:2]) + M[ids[:, 2]] * w[:, 2:3]) + M[ids[:, 3]] * w[:, 3:4]
    B = B.reshape(-1, 3, 4)
    x, y, z = rest[:, 0:1], rest[:, 1:2], rest[:, 2:3]
    return (((B[:, :, 0] * x + B[:, :, 1] * y) + B[:, :, 2] * z) + B[:, :, 3]).astype(F)
