"""glTF 2.0 ingest (.gltf + buffers, data URIs, .glb) into rsd.ingest.SceneBuilder: geometry, materials' alpha, the
camera, and what moves -- node animation, skins and morph targets (DESIGN.md 4 "glTF and morph targets").

Written against the Khronos glTF 2.0 specification (sections 3.5 scenes and nodes, 3.6 binary data, 3.7 geometry,
3.7.2.2 morph targets, 3.7.3 skins, 3.8 textures, 3.9 materials, 3.10 cameras, 3.11 and appendix C animations, 4.4
GLB); Python's standard library and numpy only.  What is read:

* containers: `.gltf` JSON whose buffers are relative files or base64 `data:` URIs; `.glb` of container version 2
  with a JSON chunk and an optional BIN chunk (buffer 0 without a uri).
* accessors: every component type, `normalized` integers (c / 255, max(c / 127, -1), ...: evaluated in float64,
  rounded to float32 once), `byteStride`, `byteOffset` on the accessor and on the bufferView.  A sparse accessor is
  refused.
* scene graph: the nodes under `scene` (the file's default scene, else scene 0; without scenes every root node); a
  node has a column-major `matrix` or translation / rotation / scale; a mesh under several nodes is one instance per
  node.  Matrices are composed in float64 and rounded once where they leave the host.
* primitives: triangles (mode 4), strips (5) and fans (6) in the specification's winding, indexed or not; points and
  lines are skipped.  Attributes POSITION, TEXCOORD_n, JOINTS_0, WEIGHTS_0; JOINTS_1 is refused.
* materials: doubleSided; alphaMode OPAQUE / MASK (alphaCutoff) / BLEND (marked Mask at 0.5, rsd.ingest's rule for
  materials whose opacity can cut holes); alpha = baseColorFactor[3] x the alpha channel of baseColorTexture (PNG; a
  JPEG has none and counts as 1) through the texCoord set it names.  Samplers must wrap by REPEAT, the one address
  mode of the alpha textures (csrc/tex_sample.h); KHR_texture_transform and other image types are refused.
* camera: the first node with a perspective camera gives position and orientation (looking down its -Z, +Y up);
  its yfov, znear and zfar are recorded in the camera dict only -- the frame's focal length and clip planes come from
  FrameConfig, as for every other importer.  Without such a node a fresh builder's camera frames the scene's bounds; a
  builder handed in (pyscene's importScene) keeps its camera.
* skins: vertex v of a skinned mesh is sum_j w_j G(joint_j) IBM_j v -- the mesh node's own transform does not act --
  one rig matrix per (skin, joint), G IBM evaluated in float64 and rounded once (AnimationController.matrices);
  weights as stored.
* animations: channels translation / rotation / scale / weights with LINEAR (rotation: slerp along the shortest arc),
  STEP and CUBICSPLINE (rotation normalised after interpolation) samplers, evaluated in float64 by the
  specification's formulas; a path without a channel keeps the node's value; every animation of the file plays at
  once; outside its keys a channel holds its first / last value (Behavior.Constant, rsd.animation's default).
* morph targets: targets[].POSITION; default weights mesh.weights, overridden by node.weights, animated by a
  `weights` channel; they become the rig's MorphTable (rsd_morph_desc).

Not read: normals and tangents (morphed or not), colours, lights, KTX / WebP images, any other extension."""
from __future__ import annotations

import base64
import json
import math
import struct
from pathlib import Path
from urllib.parse import unquote

import numpy as np

from . import animation as anim
from . import ingest

_COMPONENT = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}
_WIDTH = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT2": 4, "MAT3": 9, "MAT4": 16}
_GLB_MAGIC, _CHUNK_JSON, _CHUNK_BIN = 0x46546C67, 0x4E4F534A, 0x004E4942
_WRAP_REPEAT = 10497


class GltfError(ValueError):
    """A file this importer does not read, with the offender named."""


class GltfVersionError(GltfError, NotImplementedError):
    """A document that is not glTF 2.x (glTF 1.0, or no `asset.version` at all): there is no importer for it."""


def _label(kind, index, obj):
    return f"{kind} {index}" + (f" ('{obj['name']}')" if isinstance(obj, dict) and obj.get("name") else "")


class _File:
    """The JSON document and its buffers."""

    def __init__(self, path):
        self.path = Path(path)
        data = self.path.read_bytes()
        self.bin = None
        if data[:4] == b"glTF":
            magic, version, length = struct.unpack_from("<III", data, 0)
            if version != 2:
                raise GltfError(f"{self.path}: GLB container version {version}, not 2")
            if length > len(data):
                raise GltfError(f"{self.path}: GLB length {length} is past the file's {len(data)} bytes")
            pos, doc = 12, None
            while pos + 8 <= length:
                n, kind = struct.unpack_from("<II", data, pos)
                body = data[pos + 8:pos + 8 + n]
                if len(body) != n:
                    raise GltfError(f"{self.path}: GLB chunk at byte {pos} is cut short")
                if kind == _CHUNK_JSON and doc is None:
                    doc = body
                elif kind == _CHUNK_BIN and self.bin is None:
                    self.bin = body
                pos += 8 + n + (-n % 4)
            if doc is None:
                raise GltfError(f"{self.path}: GLB without a JSON chunk")
            self.doc = json.loads(doc.decode("utf-8"))
        else:
            self.doc = json.loads(data.decode("utf-8-sig"))
        version = str(self.doc.get("asset", {}).get("version", ""))
        if not version.startswith("2."):
            raise GltfVersionError(f"{self.path}: glTF asset version '{version}': only glTF 2.x has an importer")
        for ext in self.doc.get("extensionsRequired", []):
            raise GltfError(f"{self.path}: requires the extension {ext}, which is not read")
        self._buffers: dict[int, bytes] = {}

    def get(self, key):
        return self.doc.get(key, [])

    def uri_bytes(self, uri, what) -> bytes:
        if uri.startswith("data:"):
            head, _, body = uri.partition(",")
            if not head.endswith(";base64"):
                raise GltfError(f"{what}: a data URI that is not base64")
            return base64.b64decode(body)
        return (self.path.parent / unquote(uri)).read_bytes()

    def buffer(self, i) -> bytes:
        if i not in self._buffers:
            b = self.get("buffers")[i]
            if "uri" in b:
                raw = self.uri_bytes(b["uri"], _label("buffer", i, b))
            elif i == 0 and self.bin is not None:
                raw = self.bin
            else:
                raise GltfError(f"{_label('buffer', i, b)} has no uri and the file has no BIN chunk for it")
            if len(raw) < int(b.get("byteLength", 0)):
                raise GltfError(f"{_label('buffer', i, b)}: {len(raw)} bytes, byteLength {b['byteLength']}")
            self._buffers[i] = raw
        return self._buffers[i]

    def view_bytes(self, i) -> bytes:
        v = self.get("bufferViews")[i]
        off = int(v.get("byteOffset", 0))
        return self.buffer(v["buffer"])[off:off + int(v["byteLength"])]

    def accessor(self, i, raw=False) -> np.ndarray:
        """[count, width] in the accessor's component type; a `normalized` integer accessor as float32 (raw=False)."""
        a = self.get("accessors")[i]
        what = _label("accessor", i, a)
        if "sparse" in a:
            raise GltfError(f"{what} is sparse: sparse accessors are not read")
        dt = np.dtype(_COMPONENT[a["componentType"]]).newbyteorder("<")
        width, count = _WIDTH[a["type"]], int(a["count"])
        if a["type"].startswith("MAT") and dt.itemsize != 4:
            raise GltfError(f"{what}: a matrix accessor of {dt.itemsize}-byte components (column padding) is not read")
        if "bufferView" not in a:
            out = np.zeros((count, width), dt)
        else:
            v = self.get("bufferViews")[a["bufferView"]]
            buf = self.buffer(v["buffer"])
            start = int(v.get("byteOffset", 0)) + int(a.get("byteOffset", 0))
            stride = int(v.get("byteStride", 0)) or width * dt.itemsize
            end = start + (count - 1) * stride + width * dt.itemsize if count else start
            view_end = int(v.get("byteOffset", 0)) + int(v["byteLength"])
            if end > view_end or view_end > len(buf):
                raise GltfError(f"{what} reaches byte {end}, past its bufferView's end {min(view_end, len(buf))}")
            out = np.ndarray((count, width), dt, buf, start, (stride, dt.itemsize)).copy()
        out = out.astype(dt.newbyteorder("="))
        if a.get("normalized") and not raw and out.dtype.kind in "iu":
            top = float(np.iinfo(out.dtype).max)
            f = out.astype(np.float64) / top
            return (np.maximum(f, -1.0) if out.dtype.kind == "i" else f).astype(np.float32)
        return out


# ---------------------------------------------------------------------------------- animation

class Sampler:
    """One animation sampler (specification 3.11, appendix C): key times, key values [keys, width] -- for CUBICSPLINE
    in-tangent, value, out-tangent per key --, evaluated in float64.  Outside the keys it holds the end values."""

    def __init__(self, times, values, interpolation="LINEAR", rotation=False):
        self.times = np.asarray(times, np.float64).reshape(-1)
        n = self.times.size
        if n == 0:
            raise GltfError("an animation sampler without keys")
        if interpolation not in ("LINEAR", "STEP", "CUBICSPLINE"):
            raise GltfError(f"animation sampler interpolation '{interpolation}' is not LINEAR, STEP or CUBICSPLINE")
        v = np.asarray(values, np.float64)
        per = 3 if interpolation == "CUBICSPLINE" else 1
        if v.size % (n * per):
            raise GltfError(f"an animation sampler of {n} keys has {v.size} output values")
        self.values = v.reshape(n, per, -1)
        self.interpolation, self.rotation = interpolation, bool(rotation)

    def __call__(self, t) -> np.ndarray:
        ts, v, cubic = self.times, self.values, self.interpolation == "CUBICSPLINE"
        mid = 1 if cubic else 0
        t = float(t)
        if t <= ts[0] or ts.size == 1:
            return self._unit(v[0, mid].copy())
        if t >= ts[-1]:
            return self._unit(v[-1, mid].copy())
        k = int(np.searchsorted(ts, t, side="right")) - 1  # ts[k] <= t < ts[k + 1]
        td = ts[k + 1] - ts[k]
        u = (t - ts[k]) / td
        if self.interpolation == "STEP":
            return v[k, 0].copy()
        if not cubic:
            a, b = v[k, 0], v[k + 1, 0]
            return anim._slerp(a, b, u) if self.rotation else (1.0 - u) * a + u * b
        u2, u3 = u * u, u * u * u
        out = ((2.0 * u3 - 3.0 * u2 + 1.0) * v[k, 1] + td * (u3 - 2.0 * u2 + u) * v[k, 2]
               + (-2.0 * u3 + 3.0 * u2) * v[k + 1, 1] + td * (u3 - u2) * v[k + 1, 0])
        return self._unit(out)

    def _unit(self, q):
        if self.rotation and self.interpolation == "CUBICSPLINE":
            return q / math.sqrt(float(np.dot(q, q)))
        return q


class NodeAnimation:
    """The translation / rotation / scale channels of one node, consumed by AnimationController next to
    rsd.animation.Animation: `.nodeID`, `.animate(t)` -> the node's local float64 4x4.  A path without a channel
    keeps the node's static value."""

    def __init__(self, nodeID, translation, rotation, scale, name=""):
        self.name, self.nodeID = str(name), int(nodeID)
        self.static = {"translation": np.asarray(translation, np.float64), "rotation": np.asarray(rotation, np.float64),
                       "scale": np.asarray(scale, np.float64)}
        self.channels: dict[str, Sampler] = {}

    def value(self, path, t) -> np.ndarray:
        s = self.channels.get(path)
        return self.static[path] if s is None else s(t)

    def animate(self, t) -> np.ndarray:
        return anim.compose_trs(self.value("translation", t), self.value("rotation", t), self.value("scale", t))


class WeightAnimation:
    """The `weights` channel of one node: `.nodeID`, `.weights(t)` -> float64 [targets]."""

    def __init__(self, nodeID, sampler: Sampler, name=""):
        self.name, self.nodeID, self.sampler = str(name), int(nodeID), sampler

    def weights(self, t) -> np.ndarray:
        return self.sampler(t)


# ---------------------------------------------------------------------------------- geometry and materials

def triangle_list(mode: int, idx: np.ndarray) -> np.ndarray | None:
    """The triangles [n, 3] of a primitive's vertex sequence; None for points and lines.  Strips and fans in the
    specification's order (3.7.2.1): strip p_i = (v_i, v_(i + 1 + i % 2), v_(i + 2 - i % 2)), fan p_i = (v_(i + 1),
    v_(i + 2), v_0)."""
    idx = np.asarray(idx, np.int64).reshape(-1)
    if mode == 4:
        return idx[:idx.size // 3 * 3].reshape(-1, 3)
    n = max(idx.size - 2, 0)
    i = np.arange(n)
    if mode == 5:
        return np.stack([idx[i], idx[i + 1 + i % 2], idx[i + 2 - i % 2]], 1) if n else np.zeros((0, 3), np.int64)
    if mode == 6:
        return np.stack([idx[i + 1], idx[i + 2], np.full(n, idx[0])], 1) if n else np.zeros((0, 3), np.int64)
    if mode in (0, 1, 2, 3):
        return None
    raise GltfError(f"primitive mode {mode} is not a glTF mode")


def _image_alpha(f: _File, i: int):
    """The alpha plane uint8 [h, w] of image i, or None when the image has none (JPEG, opaque PNG)."""
    img = f.get("images")[i]
    what = _label("image", i, img)
    if "uri" in img:
        data = f.uri_bytes(img["uri"], what)
    elif "bufferView" in img:
        data = f.view_bytes(img["bufferView"])
    else:
        raise GltfError(f"{what} has neither a uri nor a bufferView")
    mime = img.get("mimeType")
    if mime is None:
        mime = "image/png" if data[:4] == b"\x89PNG" else "image/jpeg" if data[:2] == b"\xff\xd8" else None
    if mime == "image/png":
        return ingest.alpha_channel(ingest._png_decode(data), grey_is_alpha=False)
    if mime == "image/jpeg":
        return None
    raise GltfError(f"{what}: image type {mime or 'unknown'} is not read (PNG, JPEG)")


def _material(f: _File, i: int):
    """(rsd.ingest.Material, texCoord set of its alpha texture)."""
    m = f.get("materials")[i]
    what = _label("material", i, m)
    pbr = m.get("pbrMetallicRoughness", {})
    mode = m.get("alphaMode", "OPAQUE")
    if mode not in ("OPAQUE", "MASK", "BLEND"):
        raise GltfError(f"{what}: alphaMode '{mode}'")
    out = ingest.Material(name=m.get("name", f"material{i}"), double_sided=bool(m.get("doubleSided", False)),
                          alpha_mode_mask=mode != "OPAQUE",
                          alpha_threshold=float(m.get("alphaCutoff", 0.5)) if mode == "MASK" else 0.5,
                          alpha=float(pbr.get("baseColorFactor", [1.0, 1.0, 1.0, 1.0])[3]))
    tex, uv_set = pbr.get("baseColorTexture"), 0
    if tex is not None:
        if "KHR_texture_transform" in tex.get("extensions", {}):
            raise GltfError(f"{what}: baseColorTexture uses KHR_texture_transform, which is not read")
        uv_set = int(tex.get("texCoord", 0))
        t = f.get("textures")[tex["index"]]
        if "sampler" in t:
            s = f.get("samplers")[t["sampler"]]
            for key in ("wrapS", "wrapT"):
                if s.get(key, _WRAP_REPEAT) != _WRAP_REPEAT:
                    raise GltfError(f"{what}: {_label('sampler', t['sampler'], s)} has {key} {s[key]}; alpha textures "
                                    "wrap by REPEAT (10497) only")
        if "source" not in t:
            raise GltfError(f"{what}: {_label('texture', tex['index'], t)} has no source image (an extension's image?)")
        if mode != "OPAQUE":
            out.alpha_texture = _image_alpha(f, t["source"])
    return out, uv_set


def _node_trs(n):
    return (np.asarray(n.get("translation", [0.0, 0.0, 0.0]), np.float64),
            np.asarray(n.get("rotation", [0.0, 0.0, 0.0, 1.0]), np.float64),
            np.asarray(n.get("scale", [1.0, 1.0, 1.0]), np.float64))


def _node_local(n) -> np.ndarray:
    if "matrix" in n:
        return np.asarray(n["matrix"], np.float64).reshape(4, 4).T  # column-major
    return anim.compose_trs(*_node_trs(n))


# ---------------------------------------------------------------------------------- the importer

def load_gltf_builder(path, builder: ingest.SceneBuilder | None = None, scene: int | None = None) -> ingest.SceneBuilder:
    """A .gltf / .glb file into a SceneBuilder (a new one, or `builder`, like rsd.fbx.load_fbx).  scene: which of
    the file's scenes (default: the file's `scene`, else 0)."""
    f = _File(path)
    B = builder or ingest.SceneBuilder()
    nodes = f.get("nodes")
    # -- the graph: parents before children, every node of the file (a joint may sit outside the chosen scene)
    child_of = {c: i for i, n in enumerate(nodes) for c in n.get("children", [])}
    roots_all = [i for i in range(len(nodes)) if i not in child_of]
    if f.get("scenes"):
        pick = scene if scene is not None else int(f.doc.get("scene", 0))
        if not 0 <= pick < len(f.get("scenes")):
            raise GltfError(f"{f.path}: scene {pick} does not exist")
        roots = list(f.get("scenes")[pick].get("nodes", []))
    else:
        roots = roots_all
    node_id: dict[int, int] = {}
    world: dict[int, np.ndarray] = {}
    in_scene: list[int] = []

    def visit(i, parent, listed):
        if i in node_id:
            raise GltfError(f"{_label('node', i, nodes[i])} is reached twice: the node graph is not a forest")
        local = _node_local(nodes[i])
        node_id[i] = B.add_node(local, anim.INVALID_ID if parent is None else node_id[parent], dtype=np.float64)
        world[i] = local if parent is None else world[parent] @ local
        if listed:
            in_scene.append(i)
        for c in nodes[i].get("children", []):
            visit(c, i, listed)

    for r in roots:
        visit(r, None, True)
    for r in roots_all:
        if r not in node_id:
            visit(r, None, False)

    # -- materials and meshes
    materials = [_material(f, i) for i in range(len(f.get("materials")))]
    mat_ids = [B.add_material(m) for m, _ in materials]
    default_mat = None
    mesh_ids: dict[int, list] = {}

    def mesh_of(i):
        nonlocal default_mat
        if i in mesh_ids:
            return mesh_ids[i]
        g = f.get("meshes")[i]
        what = _label("mesh", i, g)
        out = []
        for k, prim in enumerate(g.get("primitives", [])):
            att = prim.get("attributes", {})
            if "JOINTS_1" in att or "WEIGHTS_1" in att:
                raise GltfError(f"{what} primitive {k} has JOINTS_1: more than 4 influences per vertex are not read")
            if "POSITION" not in att:
                continue
            pos = f.accessor(att["POSITION"]).astype(np.float32)
            idx = f.accessor(prim["indices"], raw=True).reshape(-1) if "indices" in prim else np.arange(len(pos))
            tri = triangle_list(int(prim.get("mode", 4)), idx)
            if tri is None:
                continue
            if "material" in prim:
                mat, uv_set = mat_ids[prim["material"]], materials[prim["material"]][1]
            else:
                if default_mat is None:
                    default_mat = B.add_material(ingest.Material())
                mat, uv_set = default_mat, 0
            uv = att.get(f"TEXCOORD_{uv_set}")
            mesh = ingest.Mesh(pos, tri.astype(np.uint32), None if uv is None else f.accessor(uv).astype(np.float32), mat)
            if "JOINTS_0" in att and "WEIGHTS_0" in att:
                mesh.joints = f.accessor(att["JOINTS_0"], raw=True).astype(np.uint32)
                mesh.weights = f.accessor(att["WEIGHTS_0"]).astype(np.float32)
            targets = prim.get("targets", [])
            if targets:
                mesh.morph_targets = [f.accessor(t["POSITION"]).astype(np.float32) if "POSITION" in t
                                      else np.zeros_like(pos) for t in targets]
                mesh.morph_weights = np.asarray(g.get("weights", [0.0] * len(targets)), np.float64)
            out.append(B.add_mesh(mesh))
        mesh_ids[i] = out
        return out

    skin_ids: dict[int, int] = {}

    def skin_of(i):
        if i not in skin_ids:
            s = f.get("skins")[i]
            joints = [node_id[j] for j in s["joints"]]
            ibm = None
            if "inverseBindMatrices" in s:
                m = f.accessor(s["inverseBindMatrices"]).astype(np.float64)
                if m.shape != (len(joints), 16):
                    raise GltfError(f"{_label('skin', i, s)}: {m.shape[0]} inverse bind matrices for {len(joints)} joints")
                ibm = m.reshape(-1, 4, 4).transpose(0, 2, 1)  # column-major
            skin_ids[i] = B.add_skin(joints, ibm)
        return skin_ids[i]

    camera_node = None
    for i in in_scene:
        n = nodes[i]
        if camera_node is None and "camera" in n and f.get("cameras")[n["camera"]].get("type") == "perspective":
            camera_node = i
        if "mesh" not in n:
            continue
        for mid in mesh_of(n["mesh"]):
            skinned = "skin" in n and B.meshes[mid].joints is not None
            B.add_instance(mid, None if skinned else world[i], node=node_id[i],
                           skin=skin_of(n["skin"]) if skinned else None, morph_weights=n.get("weights"))

    # -- animations: every one of the file plays; one NodeAnimation per node, a later channel of a path wins
    node_anims: dict[int, NodeAnimation] = {}
    for ai, a in enumerate(f.get("animations")):
        what = _label("animation", ai, a)
        for ch in a.get("channels", []):
            tgt = ch.get("target", {})
            if "node" not in tgt:
                continue  # a channel for an extension's target
            path, ni = tgt.get("path"), tgt["node"]
            s = a["samplers"][ch["sampler"]]
            times = f.accessor(s["input"]).astype(np.float64).reshape(-1)
            values = f.accessor(s["output"]).astype(np.float64)
            smp = Sampler(times, values, s.get("interpolation", "LINEAR"), rotation=path == "rotation")
            if path == "weights":
                B.weight_animations.append(WeightAnimation(node_id[ni], smp, a.get("name", "")))
            elif path in ("translation", "rotation", "scale"):
                if "matrix" in nodes[ni]:
                    raise GltfError(f"{what} animates {_label('node', ni, nodes[ni])}, which has a matrix instead of "
                                    "translation / rotation / scale")
                if ni not in node_anims:
                    node_anims[ni] = NodeAnimation(node_id[ni], *_node_trs(nodes[ni]), name=a.get("name", ""))
                    B.animations.append(node_anims[ni])
                node_anims[ni].channels[path] = smp
            else:
                raise GltfError(f"{what}: channel path '{path}'")

    # -- camera
    if camera_node is not None:
        M = world[camera_node]
        cam = f.get("cameras")[nodes[camera_node]["camera"]]["perspective"]
        pos = M[:3, 3]
        B.set_camera(pos, pos - M[:3, 2], M[:3, 1])
        B.camera.update(yfov=float(cam["yfov"]), znear=float(cam["znear"]),
                        zfar=float(cam["zfar"]) if "zfar" in cam else math.inf)
    elif builder is None:  # a builder handed in keeps the camera its owner set
        _frame_bounds(B)
    return B


def _frame_bounds(B: ingest.SceneBuilder):
    """Without a camera in the file: look at the centre of the static bounds from +Z, far enough to see them."""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for k, (mesh_id, T) in enumerate(B.instances):
        p = B.meshes[mesh_id].positions.astype(np.float64)
        if k not in B.instance_skins:
            p = p @ T[:3, :3].astype(np.float64).T + T[:3, 3]
        if len(p):
            lo, hi = np.minimum(lo, p.min(0)), np.maximum(hi, p.max(0))
    if not np.isfinite(lo).all():
        return
    c, r = 0.5 * (lo + hi), max(0.5 * float(np.linalg.norm(hi - lo)), 1e-3)
    B.set_camera(c + np.array([0.0, 0.0, 2.5 * r]), c)


def load_gltf(path, name: str | None = None, animated: bool = True, scene: int | None = None):
    """A .gltf / .glb file as an rsd.scenes.Scene (SceneBuilder.build of load_gltf_builder): with skins, animations
    or morph targets in the file the Scene has a rig, and GpuScene.animate(t) poses it."""
    return load_gltf_builder(path, scene=scene).build(name or Path(path).stem, animated=animated)
